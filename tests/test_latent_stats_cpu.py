"""Host side of the latent-usage statistics (lvae_amd.latent): the trainer's and the evaluation tool's flags, the suffix of a test line, the
JSONL record of such a line and the layout of the device accumulator. No GPU."""
import json

import numpy as np
import pytest


def test_parser_has_the_three_flags_with_their_defaults():
    import lvae_amd  # noqa: F401
    from lvae_amd.experiment.experiment_manager import build_parser
    a = build_parser().parse_args([])
    assert a.latent_stats is False and a.latent_kl_threshold == 0.01 and a.latent_var_threshold == 0.01
    b = build_parser().parse_args(['--latent-stats', '--latent-kl-threshold', '0.05', '--latent-var-threshold', '1e-3'])
    assert b.latent_stats is True and b.latent_kl_threshold == 0.05 and b.latent_var_threshold == 1e-3


def test_evaluate_refuses_latent_stats_without_ll(capsys):
    import lvae_amd  # noqa: F401
    from lvae_amd.evaluate import parse_eval_args
    with pytest.raises(SystemExit) as e:
        parse_eval_args(['--synthetic', '--latent-stats'])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert '--latent-stats' in err and '--ll' in err
    a = parse_eval_args(['--synthetic', '--ll', '--latent-stats', '--latent-var-threshold', '0.002'])
    assert a.latent_stats and a.ll and a.latent_var_threshold == 0.002 and a.latent_kl_threshold == 0.01
    assert parse_eval_args(['--synthetic', '--ll']).latent_stats is False


def _hand_made():
    return {'elbo/elbo': -3.0, 'n_images': 12,
            'latent/units_layer_0': 2048, 'latent/active_kl_layer_0': 1584, 'latent/active_var_layer_0': 1386,
            'latent/units_layer_1': 512, 'latent/active_kl_layer_1': 417, 'latent/active_var_layer_1': 238,
            'latent/units_layer_2': 128, 'latent/active_kl_layer_2': 87, 'latent/active_var_layer_2': 12,
            'latent/active_kl': 2088, 'latent/active_var': 1636}


def test_suffix_of_a_test_line():
    import lvae_amd  # noqa: F401
    from lvae_amd.latent import latent_line_suffix
    s = latent_line_suffix(_hand_made(), 0.01, 0.001)
    # bottom layer first, top layer last, then active / all units of the model; the same for the second measure
    assert s == ('   active units KL>0.01: 1584/2048 417/512 87/128  [2088/2688]'
                 '   var>0.001: 1386/2048 238/512 12/128  [1636/2688]')
    one = {'latent/units_layer_0': 16, 'latent/active_kl_layer_0': 0, 'latent/active_var_layer_0': 16, 'latent/active_kl': 0,
           'latent/active_var': 16}
    assert latent_line_suffix(one, 0.5, 0.25) == '   active units KL>0.5: 0/16  [0/16]   var>0.25: 16/16  [16/16]'


def test_history_keeps_the_counts_and_drops_the_arrays(tmp_path):
    import lvae_amd  # noqa: F401
    from lvae_amd.summary import History
    res = _hand_made()
    res['latent_arrays'] = [{'kl': np.zeros((8, 16, 16)), 'mu_mean': np.zeros((8, 16, 16)), 'mu_var': np.zeros((8, 16, 16))}]
    path = str(tmp_path / 'h.jsonl')
    h = History(path)
    h.write(6, 'test', res, epoch=1)
    h.close()
    rec = json.loads(open(path).read())
    assert rec['step'] == 6 and rec['split'] == 'test' and rec['epoch'] == 1
    assert 'latent_arrays' not in rec['metrics']
    want = {k: v for k, v in res.items() if k != 'latent_arrays'}
    assert rec['metrics'] == want and all(isinstance(rec['metrics'][k], int) for k in want if k.startswith('latent/'))


def test_layout_of_a_three_layer_model_needs_no_device():
    import lvae_amd  # noqa: F401
    from lvae_amd import latent
    from lvae_amd.models.lvae import LadderVAE
    m = LadderVAE(3, [32, 32, 32], downsample=[1, 1, 1], merge_type='residual', n_filters=8, dropout=0.1, img_shape=(32, 32),
                  likelihood_form='discr_log_mix', res_block_type='bacdbacd', gated=True)
    shapes = latent.layer_shapes(m)
    assert shapes == [(32, 8, 8), (32, 4, 4), (32, 2, 2)]                  # the stem halves the image, then every layer once more
    offsets, total = latent.layout(shapes)
    # slot 0 is the image count; a layer owns three runs of its U units
    assert offsets == [1, 1 + 3 * 2048, 1 + 3 * 2048 + 3 * 512] and total == 1 + 3 * (2048 + 512 + 128)
    # no initial downscaling, a layer that keeps its size, unequal z_dims
    m2 = LadderVAE(1, [4, 6], downsample=[0, 1], merge_type='residual', n_filters=8, dropout=0.1, img_shape=(28, 28),
                   likelihood_form='bernoulli', res_block_type='bacdbacd', gated=True, no_initial_downscaling=True)
    assert latent.layer_shapes(m2) == [(4, 28, 28), (6, 14, 14)]
    assert latent.layout(latent.layer_shapes(m2)) == ([1, 1 + 3 * 4 * 784], 1 + 3 * 4 * 784 + 3 * 6 * 196)


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    """The argument checks return LVAE_EINVAL before any HIP call, so they can be exercised without a GPU (the pointers are never read)."""
    import lvae_amd  # noqa: F401
    from lvae_amd import _C
    lib = _C.load()
    N, HW, Z = 8, 16, 32
    need = lib.lvae_latent_stats_workspace(N, HW, Z)
    assert need >= 3 * HW * Z * 8 and need % (3 * HW * Z * 8) == 0               # whole slices of [3][U] doubles
    assert lib.lvae_latent_stats_workspace(0, HW, Z) == lib.lvae_latent_stats_workspace(N, 0, Z) == lib.lvae_latent_stats_workspace(N, HW, -1) == 0
    assert lib.lvae_latent_stats_workspace(1000, 256, 32) < 1000 * 256 * 64 * 4  # the partials stay below one tensor of the batch
    fake = 0x1000
    bad = [(fake, 0, fake, N, HW, Z, fake, fake, need - 1, None),                # one byte short
           (fake, 0, fake, 0, HW, Z, fake, fake, need, None), (fake, 0, fake, N, 0, Z, fake, fake, need, None),
           (fake, 0, fake, N, HW, 0, fake, fake, need, None),
           (None, 0, fake, N, HW, Z, fake, fake, need, None), (fake, 0, None, N, HW, Z, fake, fake, need, None),
           (fake, 0, fake, N, HW, Z, None, fake, need, None), (fake, 0, fake, N, HW, Z, fake, None, need, None)]
    for args in bad:
        assert lib.lvae_latent_stats_fold_f32(*args) == -1, args
        assert b'lvae_latent_stats_fold_f32' in lib.lvae_last_error()
        with pytest.raises(_C.LvaeHipError):
            _C.call('lvae_latent_stats_fold_f32', *args)
    for args in [(fake, 512, 0, 0.01, 0.01, fake, fake, None), (fake, 512, -3, 0.01, 0.01, fake, fake, None),
                 (fake, 0, 4, 0.01, 0.01, fake, fake, None), (None, 512, 4, 0.01, 0.01, fake, fake, None)]:
        assert lib.lvae_latent_stats_finalize_f64(*args) == -1, args
