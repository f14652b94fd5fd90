"""Two exact savings of the fp16x2 DIEN scorer, pinned:

* the dense tower and the q-side term of the DIN scores as ONE launch (k_gemm_h16_pair) against the two launches of
  scorer_kernels='no_gemm_group': same tile, k-blocks, MFMA order and epilogue per output element - bit-identical;
* k_augru_x without the vanishing products of its boundary steps (step 0: h = 0, so items 0-39 multiply zeros; last step: the
  reset-gate product of a step that does not exist) at history lengths where the first step is far from, next to and equal to
  the last one, in the 32-row (with and without the pad-slot redirect) and the 64-row form, every row against the fp64 oracle
  at the bars of tests/test_gpu_dien.py (AUGRU final states 5e-6, observation 5e-5, click probability 5e-6 abs)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32}


def _histories(B, L, rs):
    """[B, 2, L] ids: a third of the rows of input 0 start with padding (half the history, at least one step), every second
    row of input 1 is all padding, the rest have no zero id at all."""
    seq = rs.randint(1, 284, size=(B, 2, L)).astype(np.int32)
    seq[: B // 3, 0, : max(1, L // 2)] = 0
    seq[::2, 1, :] = 0
    return seq


def _rows(R, rs, hash_size):
    dense = np.abs(rs.randn(R, 432) * 3).astype(np.float32)
    cat = rs.randint(0, hash_size, size=(R, 21)).astype(np.int32)
    cat[:, 10:] = rs.randint(0, 284, size=(R, 11))
    return dense, cat


@pytest.mark.parametrize('precision,R,group,extra', [('fp16x2', 4096, 1, ''), ('fp16x2', 300, 1, ''), ('fp16x2', 33, 1, ''),
                                                      ('fp16x2', 32800, 8, ''), ('fp16x2', 300, 1, 'no_dense_chain'),
                                                      ('fp32', 300, 1, '')])
def test_grouped_gemm_launch_is_bit_identical(precision, R, group, extra):
    """Default handle (dense tower + q-side term in one launch) against scorer_kernels='no_gemm_group': observation, click
    probability, the all-feature buffer (the dense tower's columns among them) and the attention scores (a function of the
    q-side product) bit for bit.  R = 4096: one workgroup per CU; 300 / 33: ragged last row tile; 32800 rows in groups of 8:
    past the 32-row-tile threshold of k_gemm_h16 (64-row tiles, ragged); with 'no_dense_chain' and in fp32 mode there is
    nothing to group: the option must be a no-op."""
    import torch
    from rl4rs_amd.nets.dien import init_dien_weights
    from rl4rs_amd.device import DeviceDien, DIEN_ALL_FEATURE, DIEN_SCORES
    cfg = dict(CFG, scorer_precision=precision)
    B = R // group
    w = init_dien_weights(cfg, seed=9, emb_scale=0.5, bias_noise=0.2)
    rs = np.random.RandomState(R)
    nslots = min(B, 512)                                   # histories are shared between envs: the GEMMs under test do not read them
    seq = _histories(nslots, 64, rs)
    dense, cat = _rows(R, rs, cfg['category_hash_size'])
    sl = torch.from_numpy((np.arange(B) % nslots).astype(np.int32)).repeat(2, 1).contiguous().cuda()

    def run(kernels):
        net = DeviceDien(dict(cfg, scorer_kernels=kernels), w, max_rows=R, max_slots=nslots)
        assert net.scorer_mode == precision
        for s in range(2):
            net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
        obs, p = net.forward(R, group, torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda(), sl, True, True)
        out = (obs.clone(), p.clone(), net.snapshot(DIEN_ALL_FEATURE, R)[:R].clone(), net.snapshot(DIEN_SCORES, R)[:, :R].clone())
        labels = sorted(net.profile())
        net.close()
        return out, labels

    ref, labels_ref = run(extra)
    two, labels_two = run(','.join(x for x in ('no_gemm_group', extra) if x))
    grouped = precision == 'fp16x2' and not extra
    assert any('k_gemm_h16_pair' in k for k in labels_ref) == grouped, labels_ref
    assert not any('k_gemm_h16_pair' in k for k in labels_two), labels_two
    assert any('q-side term' in k and 'k_din' in k for k in labels_two), labels_two
    assert torch.isfinite(ref[0]).all() and torch.isfinite(ref[1]).all()
    for name, a, b in zip(('obs', 'prob', 'all_feature', 'scores'), ref, two):
        print(name, 'max |grouped - two launches| =', (a - b).abs().max().item())
        assert torch.equal(a, b), name


@pytest.mark.parametrize('kernels', ['', 'no_gru_pad'])
@pytest.mark.parametrize('L', [64, 33, 16, 2, 1])
def test_augru_boundary_steps_against_the_oracle(L, kernels):
    """R = 576 rows in groups of 8 per cache slot (nine 64-row tiles, eighteen 32-row tiles), histories with and without leading
    padding: the 64-row form, then the 32-row form over the same cache (default handle: its pad-slot instantiation;
    'no_gru_pad': the plain one) - EVERY row's AUGRU final states, observation and click probability against the fp64 oracle,
    and the two forms bit-identical to each other.  maxlen 2: the first step is followed by the last; maxlen 1: one step is
    both."""
    import torch
    from rl4rs_amd.nets.dien import init_dien_weights
    from rl4rs_amd.device import DeviceDien, DIEN_ALL_FEATURE
    from oracle.dien import OracleDien
    cfg = dict(CFG, maxlen=L, scorer_precision='fp16x2', scorer_kernels=kernels)
    B, G = 72, 8
    R = B * G
    w = init_dien_weights(cfg, seed=13, emb_scale=0.5, bias_noise=0.2)
    rs = np.random.RandomState(100 + L)
    seq_env = _histories(B, L, rs)
    dense, cat = _rows(R, rs, cfg['category_hash_size'])
    net = DeviceDien(cfg, w, max_rows=R, max_slots=B)
    assert net.scorer_mode == 'fp16x2' and net.augru_kernel == 'k_augru_x'
    for s in range(2):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(seq_env[:, s])).cuda(), 0)
    sl = torch.arange(B, dtype=torch.int32).repeat(2, 1).contiguous().cuda()
    d, c = torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
    seq_rows = np.repeat(seq_env, G, axis=0)
    orc = OracleDien(w, cfg, np.float64)
    _, parts = orc.features(seq_rows, dense, cat, return_parts=True)
    obs_ref = orc.obs(seq_rows, dense, cat)
    prob_ref = orc.reward_probs(seq_rows, dense, cat)[:, 1]
    got = {}
    for rows in (64, 32):
        net.set_augru_rows(rows)
        obs, p = net.forward(R, G, d, c, sl, True, True)
        af = net.snapshot(DIEN_ALL_FEATURE, R)[:R, :512].clone()
        got[rows] = (obs.clone(), p.clone(), af)
        a = af.cpu().numpy()
        e0, e1 = np.abs(a[:, :256] - parts['h2_0']).max(), np.abs(a[:, 256:512] - parts['h2_1']).max()
        eo, ep = np.abs(obs.cpu().numpy() - obs_ref).max(), np.abs(p.cpu().numpy() - prob_ref).max()
        print('L=%d %s rows=%d: h2_0 %.3g h2_1 %.3g obs %.3g prob %.3g' % (L, kernels or 'default', rows, e0, e1, eo, ep))
        assert e0 < 5e-6 and e1 < 5e-6, rows
        assert eo < 5e-5, rows
        assert ep < 5e-6, rows
    for x64, x32 in zip(got[64], got[32]):
        assert torch.equal(x64, x32)
    net.check_status()
    net.close()
