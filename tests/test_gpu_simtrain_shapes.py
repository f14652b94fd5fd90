"""Simulator training away from the reference's default configuration (E = U = 128, maxlen 64, two sequence inputs, two
classes, 21 categories, 432 dense features - the only one tests/test_gpu_simtrain.py runs): every gradient of
rl4rs_dientrain_grad / rl4rs_simtrain_grad against torch float64 autograd at E != U, odd widths, lengths 1 / 16 / 33 / 80,
1 / 3 / 4 sequence inputs, 3 / 8 classes, the DIEN trainer's own minibatch (256), every row-tile form of the persistent
recurrences, both GRU paths of the lstm trainer; every GRU implementation of the lstm trainer with keras hard_sigmoid gates on
both clamps (no other input of these files reaches +-2.5: tests/test_simnet_shapes_host.py); the trainer -> scorer hand-off; the DIEN
trainer's create-time limits.
Same bars as tests/test_gpu_simtrain.py: loss 1e-5 relative, gradients 2e-4 (simnets) / 5e-4 (dien) of each array's largest
entry, scorer obs 5e-5 and probabilities 5e-6 absolute."""
import numpy as np
import pytest

from simnet_cases import SHAPES, scale_gru
from test_gpu_simtrain import CFG, DIEN_CFG, _check_dien_gradients, _check_simnet_gradients, recur_rows  # noqa: F401

pytestmark = pytest.mark.gpu

# row-tile form of the persistent recurrences: 0 = automatic, 4 (hidden width 256; width 128 takes 8), 8, 32 = pinned
ROWS = [0, 4, 8, 32]

# DIEN trainer configurations (emb_size 128 and category_feature_num >= 10 are the trainer's own limits): the first GRU is 128
# wide, the AUGRU 256, both with sigmoid gates
DIEN_VARIANTS = {
    'D1': dict(DIEN_CFG, maxlen=33, category_feature_num=13, hidden_units=96, dense_feature_num=61, seq_num=3, class_num=3),
    'D2': dict(DIEN_CFG, maxlen=16, category_feature_num=32, hidden_units=128, dense_feature_num=40, seq_num=2),   # L < 32, top of Cn
    'D3': dict(DIEN_CFG, maxlen=64, category_feature_num=10, hidden_units=32, seq_num=1),          # one input: no second stream
    'D4': dict(DIEN_CFG, maxlen=1, category_feature_num=10, seq_num=4, class_num=8),             # one step; two inputs per stream
}

# dnn / widedeep / lstm at the scorer's odd configuration (tests/test_gpu_simnet.py::test_simnet_other_configuration)
ODD = dict(CFG, emb_size=72, hidden_units=96, dense_feature_num=61, category_feature_num=13, seq_num=3, class_num=3, maxlen=33)


@pytest.mark.parametrize('rows', ROWS)
def test_dien_gradients_at_the_training_minibatch(recur_rows, rows):
    """N = 256, the minibatch SimulatorTrainer trains with: automatically the AUGRU in 4-row and the first GRU in 8-row workgroups"""
    recur_rows(rows)
    _check_dien_gradients(0.2, 256)


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('name', sorted(DIEN_VARIANTS))
def test_dien_gradients_other_configurations(recur_rows, name, rows):
    """N = 43: ragged last tile of every row form; dropout 0.2 (keep masks [N, hidden_units])"""
    recur_rows(rows)
    _check_dien_gradients(0.2, 43, DIEN_VARIANTS[name])


@pytest.mark.parametrize('name', sorted(DIEN_VARIANTS))
def test_dien_gradients_single_row(name):
    _check_dien_gradients(0.2, 1, DIEN_VARIANTS[name])


def test_dien_gradients_on_one_stream():
    """rl4rs_dientrain_set_fork(0): the odd inputs' chains on the caller's stream - same gradients, same bars"""
    from rl4rs_amd import _lib
    lib = _lib.load()
    _lib.check(lib.rl4rs_dientrain_set_fork(0))
    try:
        _check_dien_gradients(0.2, 43, DIEN_VARIANTS['D1'])
    finally:
        _lib.check(lib.rl4rs_dientrain_set_fork(1))


@pytest.mark.parametrize('algo', ['dnn', 'widedeep'])
@pytest.mark.parametrize('rate', [0.0, 0.2])
def test_simnet_gradients_other_configuration(algo, rate):
    _check_simnet_gradients(algo, rate, 43, ODD, front_pad=True)


def _gru_persistent(cfg, N):
    """simtrain.hpp gru_persistent(), restated: the lstm trainer's GRUs run as the persistent recurrences (recur_train.hpp,
    recur8.hpp) iff hidden_units is 128 or 256 and, for BOTH lengths - the category GRU's (category_feature_num steps) and the
    sequence GRUs' (maxlen) - len <= 64 and N * len * 3 * hidden_units * 4 < 2^31 bytes; otherwise every GRU takes the
    step-by-step form (k_gru_gates / k_gru_update forwards, k_gru_bwd_pre / k_gru_bwd_mid backwards, GEMMs between)"""
    U = cfg['hidden_units']
    return U in (128, 256) and all(n <= 64 and N * n * 3 * U * 4 < 2 ** 31 for n in (cfg['category_feature_num'], cfg['maxlen']))


LSTM_VARIANTS = {
    # width 256 with keras hard_sigmoid gates: k_recur8_fwd/bwd<256,4>, <256,8>, k_recur<256,..>/k_recur_bwd<256> with hard = 1
    'w256': (dict(CFG, hidden_units=256), True),
    # step-by-step by width (96 is not 128 / 256)
    'steps_width': (dict(ODD), False),
    # step-by-step by length (maxlen 80 > 64)
    'steps_length': (dict(CFG, maxlen=80), False),
    # persistent width 128 with category GRUs of 13 and 32 steps
    'w128_cn13': (dict(CFG, category_feature_num=13, maxlen=33), True),
    'w128_cn32': (dict(CFG, category_feature_num=32, maxlen=33), True),
}


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('N', [256, 43])
def test_lstm_gradients_width_256_hard_gates(recur_rows, N, rows):
    cfg, persistent = LSTM_VARIANTS['w256']
    assert _gru_persistent(cfg, N) and persistent
    recur_rows(rows)
    _check_simnet_gradients('lstm', 0.2, N, cfg, front_pad=True)


@pytest.mark.parametrize('name', ['steps_width', 'steps_length', 'w128_cn13', 'w128_cn32'])
def test_lstm_gradients_other_configurations(name):
    cfg, persistent = LSTM_VARIANTS[name]
    N = 43
    assert _gru_persistent(cfg, N) == persistent, name
    _check_simnet_gradients('lstm', 0.2, N, cfg, front_pad=True)


# keras hard_sigmoid gates on both clamps: the GRU matrices of the seeded weights times 8 (simnet_cases.scale_gru) put about a third
# of the gate pre-activations beyond +-2.5, where the gate's derivative is 0 instead of 0.2.  N = 9: two 8-row tiles, three 4-row
# tiles, one 32-row tile - the last one ragged in every form; maxlen 4, 3 categories; no dropout (the probability condition below is
# then a statement about the restatement alone).  name -> (configuration, persistent, seed of the weights and of the batch).  The
# gradient is discontinuous at the kinks, so a seed qualifies only if, in the float64 restatement, no gate pre-activation lies closer
# to +-2.5 than 10 x the largest float32-vs-float64 difference of one, and every class probability stays inside [1e-6, 1 - 1e-6]
# (the loss clamp is no second kink).  tests/test_simnet_shapes_host.py checks both on the CPU; measured there:
#   w128  seed 10: kink margin 4.6e-4, float32 pre-activation error 9.3e-6, saturated 18.4 % / 18.4 %
#   w256  seed 14: kink margin 2.6e-4, float32 pre-activation error 9.7e-6, saturated 15.4 % / 16.0 %
#   steps seed 7: kink margin 6.3e-4, float32 pre-activation error 7.0e-6, saturated 17.9 % / 17.1 %
# (of seeds 0..19, 10 / 7 / 16 qualify; these have the widest margin.)  float32 autograd of the restatement on these cases: loss off
# by at most 1.5e-7, a gradient array by at most 3.1e-6 of its largest entry - under a quarter of the bars, so the file's own hold.
SATURATED_N = 9
SATURATED = {
    'w128': (dict(CFG, maxlen=4, category_feature_num=3), True, 10),
    'w256': (dict(CFG, hidden_units=256, maxlen=4, category_feature_num=3), True, 14),
    'steps': (dict(CFG, emb_size=72, hidden_units=96, maxlen=4, category_feature_num=3), False, 7),
}


def saturated_case(name):
    """-> the arguments of _simnet_case / _check_simnet_gradients for one saturated-gate case"""
    cfg, _, seed = SATURATED[name]
    return dict(algo='lstm', rate=0.0, N=SATURATED_N, cfg=cfg, front_pad=True, seed=seed, input_seed=seed, weight_hook=scale_gru)


@pytest.mark.parametrize('name,rows', [('w128', 0), ('w128', 8), ('w128', 32), ('w256', 0), ('w256', 4), ('w256', 8), ('w256', 32),
                                       ('steps', 0)])
def test_lstm_gradients_with_saturated_gates(recur_rows, name, rows):
    """every GRU implementation of the lstm trainer with gates on both clamps of hard_sigmoid: the persistent recurrences at width 128
    (8- and 32-row tiles) and 256 (4-, 8- and 32-row tiles; 0 = what the library picks itself), and the step-by-step form (E 72, U 96).
    Bars: the file's own; a figure the float32 autograd of the restatement itself misses by more than a quarter of its bar takes 4 x that
    miss (_check_simnet_gradients prints every such figure)."""
    cfg, persistent, _ = SATURATED[name]
    assert _gru_persistent(cfg, SATURATED_N) == persistent, name
    recur_rows(rows)
    _check_simnet_gradients(**saturated_case(name))


@pytest.mark.parametrize('algo', ['dnn', 'widedeep', 'dien', 'lstm'])
def test_trained_weights_drop_into_the_scorer(algo):
    """Trainer -> scorer at an odd configuration (dnn / widedeep: ODD, dien: D1, lstm: L3 of simnet_cases - E = U = 128 as its
    scorer requires): one step() is keras Adam's first update of
    every array; after three steps weights() - the export layout - loads into DeviceSimnet / DeviceDien at the same configuration,
    whose obs / probabilities match the float64 oracle of those exported weights (dien: both scorer modes)."""
    import torch
    from rl4rs_amd.device import DeviceSimTrainer, DeviceDienTrainer, DeviceSimnet, DeviceDien
    cfg = DIEN_VARIANTS['D1'] if algo == 'dien' else (SHAPES['L3'][1] if algo == 'lstm' else ODD)
    L, S, Cn, Dn, K = cfg['maxlen'], cfg['seq_num'], cfg['category_feature_num'], cfg['dense_feature_num'], cfg['class_num']
    N = 45
    if algo == 'dien':
        from rl4rs_amd.nets.dien import init_dien_weights
        w = init_dien_weights(cfg, seed=5, emb_scale=0.5, bias_noise=0.2)
        tr = DeviceDienTrainer(cfg, w, max_batch=N)
    else:
        from rl4rs_amd.nets.simnets import init_simnet_weights
        w = init_simnet_weights(cfg, algo, seed=9, emb_scale=0.4, bias_noise=0.2)
        tr = DeviceSimTrainer(cfg, w, max_batch=N, algo=algo)
    rs = np.random.RandomState(11)
    seq = rs.randint(0, 284, size=(N, S, L)).astype(np.int32)
    seq[: N // 3, 0, : L // 2] = 0
    seq[::2, 1, :] = 0
    dense = np.abs(rs.randn(N, Dn)).astype(np.float32)
    cat = rs.randint(0, cfg['category_hash_size'], size=(N, Cn)).astype(np.int32)
    cat[:, Cn - 11:] = rs.randint(0, 284, size=(N, 11))
    labels = rs.randint(0, K, size=N).astype(np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dd, dc, dl, ds = t(dense), t(cat), t(labels), [t(seq[:, s]) for s in range(S)]
    before = dict((k, v.clone()) for k, v in tr.weights().items())
    assert set(before) == set(w)
    for k in w:
        assert np.array_equal(before[k].cpu().numpy(), w[k]), k           # the import layout
    tr.grad(dd, dc, dl, ds, dropout_rate=0.0)
    g = tr.gradients()
    assert tr.iteration == 0
    tr.step(dd, dc, dl, ds, lr=1e-3, dropout_rate=0.0)
    after = tr.weights()
    # keras Adam, first step (m = v = 0): w -= lr_t * (1 - b1) g / (sqrt((1 - b2) g^2) + eps), lr_t = lr sqrt(1 - b2) / (1 - b1)
    lr_t = 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)
    for k in before:
        expect = before[k] - lr_t * (0.1 * g[k]) / (torch.sqrt(0.001 * g[k] * g[k]) + 1e-7)
        assert torch.allclose(after[k], expect, rtol=0, atol=2e-6), k
    for _ in range(2):
        tr.step(dd, dc, dl, ds, lr=1e-3, dropout_rate=0.2, seed=4)
    trained = dict((k, v.cpu().numpy()) for k, v in tr.weights().items())
    tr.close()
    for k in w:
        assert trained[k].shape == w[k].shape and not np.array_equal(trained[k], w[k]), k      # every array trained
    slots = torch.arange(N, dtype=torch.int32).repeat(S, 1).contiguous().cuda()
    if algo == 'dien':
        from oracle.dien import OracleDien
        orc = OracleDien(trained, cfg, np.float64)
        nets = [DeviceDien(dict(cfg, scorer_precision=mode), trained, max_rows=N, max_slots=N) for mode in ('fp32', 'fp16x2')]
    else:
        from oracle.simnets import OracleSimnet
        orc = OracleSimnet(algo, trained, cfg, np.float64)
        nets = [DeviceSimnet(cfg, trained, max_rows=N, max_slots=N, algo=algo)]
    obs_ref = orc.obs(seq, dense, cat)
    prob_ref = orc.reward_probs(seq, dense, cat)[:, 1]
    for net in nets:
        for s in range(S):
            net.encode(s, ds[s], 0)
        obs, prob = net.forward(N, 1, dd, dc, slots, want_obs=True, want_prob=True)
        assert np.abs(obs.cpu().numpy() - obs_ref).max() < 5e-5
        assert np.abs(prob.cpu().numpy() - prob_ref).max() < 5e-6
        net.close()


def test_dien_trainer_refuses_shapes_beyond_its_recurrences():
    """At create (never at a first grad): maxlen > 64, and a max_batch whose AUGRU pre-activations reach 2^31 bytes"""
    from rl4rs_amd.nets.dien import init_dien_weights
    from rl4rs_amd.device import DeviceDienTrainer
    from rl4rs_amd._lib import Rl4rsHipError
    w = init_dien_weights(DIEN_CFG, seed=3)
    with pytest.raises(Rl4rsHipError, match='maxlen must be <= 64'):
        DeviceDienTrainer(dict(DIEN_CFG, maxlen=65), w, max_batch=8)
    with pytest.raises(Rl4rsHipError, match=r'max_batch 10923 too large.*max_batch <= 10922 at maxlen 64'):
        DeviceDienTrainer(DIEN_CFG, w, max_batch=10923)
