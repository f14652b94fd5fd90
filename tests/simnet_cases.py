"""Case generators shared by tests/test_gpu_simnet_shapes.py (device), tests/test_gpu_simtrain_shapes.py (device) and
tests/test_simnet_shapes_host.py (CPU): the off-default configurations of the dnn / widedeep / lstm scorer, their seeded inputs,
the x8 GRU matrices that saturate keras hard_sigmoid gates, and the float32-restatement yardstick of a bar.  numpy only."""
import numpy as np

BASE = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
        "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
        "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32}

# what rl4rs_simnet_create states (csrc/simnet.hpp): inclusive ranges and divisors
CREATE_RANGES = {'maxlen': (1, 64), 'category_feature_num': (1, 64), 'seq_num': (1, 4), 'class_num': (1, 8)}
CREATE_MULTIPLES = {'emb_size': 8, 'hidden_units': 32}
LSTM_WIDTH = 128            # lstm: emb_size == hidden_units == 128 (the recurrent kernel's own limit)

# name -> (algo, configuration)
SHAPES = {
    'L1': ('lstm', dict(BASE, maxlen=1, category_feature_num=1, seq_num=1, dense_feature_num=1, class_num=3)),
    'L2': ('lstm', dict(BASE, maxlen=33, category_feature_num=64, seq_num=4, dense_feature_num=61, class_num=8,
                        category_hash_size=7)),
    'L3': ('lstm', dict(BASE, maxlen=16, category_feature_num=13, seq_num=3, dense_feature_num=40, class_num=2)),
    'D1': ('dnn', dict(BASE, emb_size=8, hidden_units=32, category_feature_num=1, dense_feature_num=1, class_num=8)),
    'D2': ('dnn', dict(BASE, emb_size=200, hidden_units=160, category_feature_num=64, dense_feature_num=500, class_num=3)),
    'W1': ('widedeep', dict(BASE, emb_size=8, hidden_units=32, category_feature_num=1, dense_feature_num=1, seq_num=1,
                            maxlen=1, class_num=8)),
    'W2': ('widedeep', dict(BASE, emb_size=200, hidden_units=160, category_feature_num=64, dense_feature_num=500, seq_num=4,
                            maxlen=33, class_num=3)),
    'L0': ('lstm', dict(BASE)),           # the default configuration
}
TABLE = ['L1', 'L2', 'L3', 'D1', 'D2', 'W1', 'W2']
TABLE_R = 65
# one configuration per family over the row-count edges: 4-row gather / head blocks, 32-row k_recur blocks, max_rows = R
ROW_SWEEP = {'lstm': 'L0', 'dnn': 'D2', 'widedeep': 'W2'}
ROW_COUNTS = [1, 31, 32, 33, 65]
SATURATED = ['L0', 'L3']      # forward cases with scaled GRU matrices, R = 65
GRU_SCALE = 8.0
# (factor of every *_gru_kernel, of every *_gru_recurrent).  'x8': both times 8 - over 64 steps that recurrence amplifies rounding
# (float32 and float64 restatements part ways), so its bar is mostly the yardstick's; 'kernel16': the input side alone times 16
# saturates as many gates and keeps the recurrence contractive, so the fixed bars hold
SAT_VARIANTS = {'x8': (GRU_SCALE, GRU_SCALE), 'kernel16': (16.0, 1.0)}

OBS_BAR, PROB_BAR = 5e-5, 5e-6       # tests/test_gpu_simnet.py's bars


def scale_gru(w, kernel=GRU_SCALE, recurrent=GRU_SCALE):
    """every *_gru_kernel times `kernel`, every *_gru_recurrent times `recurrent` (biases untouched): trained-size gate
    pre-activations"""
    out = dict((k, np.array(v, copy=True)) for k, v in w.items())
    for k in out:
        if k.endswith('_gru_kernel'):
            out[k] = (out[k] * np.float32(kernel)).astype(np.float32)
        elif k.endswith('_gru_recurrent'):
            out[k] = (out[k] * np.float32(recurrent)).astype(np.float32)
    return out


def weights(name, seed=3, saturated=None):
    """saturated: None or a key of SAT_VARIANTS"""
    from rl4rs_amd.nets.simnets import init_simnet_weights
    algo, cfg = SHAPES[name]
    w = init_simnet_weights(cfg, algo, seed=seed, emb_scale=0.5, bias_noise=0.2)
    return scale_gru(w, *SAT_VARIANTS[saturated]) if saturated else w


def inputs(cfg, R, seed):
    """seq [R, S, L] i32, dense [R, Dn] f32, cat [R, Cn] i32.  Ids are drawn from the whole table; id 0 and id H - 1 both occur in
    `cat` and in every sequence input whenever it holds at least two entries (front padding and an all-zero history as in
    tests/test_gpu_simnet.py)."""
    rs = np.random.RandomState(seed)
    L, S, Cn, Dn, H = cfg['maxlen'], cfg['seq_num'], cfg['category_feature_num'], cfg['dense_feature_num'], cfg['category_hash_size']
    seq = rs.randint(0, H, size=(R, S, L)).astype(np.int32)
    seq[: R // 3, 0, : L // 3] = 0
    if S > 1:
        seq[::2, 1, :] = 0
    dense = np.abs(rs.randn(R, Dn) * 3).astype(np.float32)
    cat = rs.randint(0, H, size=(R, Cn)).astype(np.int32)
    flat = cat.reshape(-1)
    flat[0] = 0
    flat[-1] = H - 1
    for s in range(S):
        seq[0, s, 0] = 0
        seq[R - 1, s, L - 1] = H - 1
    return seq, dense, cat


def case_inputs(name, R=TABLE_R):
    return inputs(SHAPES[name][1], R, seed=1000 + R)


def yardstick(algo, w, cfg, seq, dense, cat):
    """-> (obs_ref, prob_ref [R], e_obs, e_prob): the float64 restatement and what float32 alone costs on these inputs"""
    from oracle.simnets import OracleSimnet
    o64 = OracleSimnet(algo, w, cfg, np.float64)
    o32 = OracleSimnet(algo, w, cfg, np.float32)
    obs64, obs32 = o64.obs(seq, dense, cat), o32.obs(seq, dense, cat)
    p64 = o64.reward_probs(seq, dense, cat)[:, 1]
    p32 = o32.reward_probs(seq, dense, cat)[:, 1]
    return obs64, p64, float(np.abs(obs32 - obs64).max()), float(np.abs(p32 - p64).max())


def bar(fixed, e32):
    """the fixed bar, unless float32 alone costs more than a quarter of it on the case's own inputs: then 4 x that cost (the suite's
    factor for a different accumulation order).  Never a function of device output."""
    return fixed if e32 <= fixed / 4 else 4 * e32


def gate_stats(algo, w, cfg, seq, dense, cat):
    """lstm -> (pre64, e_pre): float64 gate pre-activations (flat) and the largest float32-vs-float64 difference of one"""
    from oracle.simnets import OracleSimnet
    p64 = OracleSimnet(algo, w, cfg, np.float64).gate_preacts(seq, dense, cat)
    p32 = OracleSimnet(algo, w, cfg, np.float32).gate_preacts(seq, dense, cat)
    return p64, float(np.abs(p32.astype(np.float64) - p64).max())


def kink_margin(pre):
    """distance of the closest gate pre-activation to a hard_sigmoid kink (+-2.5)"""
    return float(np.abs(np.abs(pre) - 2.5).min())


# the episode off the default: maxlen 16, ten envs; histories of 1 .. 40 items
EPISODE_MAXLEN, EPISODE_B = 16, 10


def episode_records():
    """-> catalog text, EPISODE_B + 5 log records (one page)"""
    from rl4rs_amd import synth
    cat_text = synth.make_catalog_text(seed=21)
    return cat_text, synth.make_records(EPISODE_B + 5, pages=1, seed=8, illegal_frac=0.3, hash_size=5000, max_hist=40,
                                        special_ids=synth.special_ids_from_text(cat_text))


def history_lengths(records):
    """items in the history field (the sixth of a record's '@'-separated fields)"""
    return [len(r.split('@')[5].split(',')) for r in records]
