"""The row builder of replay-ahead (k_env_rows_ahead, env.hip) against oracle/state.py: behind the act of step c0 the
kernel writes, for every env, the state rows of the acts c0 .. c0 + n - 1 under the logged actions.  The oracle is stepped through
those actions; every dense and category row must be equal exactly (copies and integers).  B = 5 (one partial workgroup) and B = 70
(more than one), T = 9 and T = 10, c0 = 0 behind a logged and c0 = 1 behind a random first action (prev_actions up to c0 are the
env's own), 8 rows per env and every row that is left."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('T', [9, 10])
@pytest.mark.parametrize('B', [5, 70])
def test_rows_equal_the_oracle_stepped_through_the_logged_actions(tmp_path, B, T):
    from rl4rs_amd import synth
    from rl4rs_amd.data import CatalogTables, RecordColumns
    from rl4rs_amd.device import DeviceEnv
    from oracle.state import OracleState
    cat_path = os.path.join(str(tmp_path), 'item_info.csv')
    cat_text = synth.make_catalog_text(seed=99)
    synth.write_text(cat_path, cat_text)
    records = synth.make_records(B, pages=2 if T > 9 else 1, seed=5, illegal_frac=0.3, special_ids=synth.special_ids_from_text(cat_text))
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 100000, "seq_num": 2, "emb_size": 128, "page_items": 9, "hidden_units": 128, "max_steps": T,
           "action_emb_size": 32, "iteminfo_file": cat_path}
    rs = np.random.RandomState(3)
    for c0 in (0, 1):
        for n in sorted({8, T - 1 - c0, T - c0}):
            cols = RecordColumns(records, cfg['maxlen'])
            env = DeviceEnv(cfg, CatalogTables(cat_path, 284, 32, False), False, cols.log_steps, True)
            env.load_batch(cols.exposed, cols.feedback, cols.history, cols.user_dense, cols.user_cat)
            env.reset()
            st = OracleState(cfg, records, seq=False)
            for t in range(c0 + 1):
                a = np.asarray(st.offline_action) if c0 == 0 else rs.randint(0, 284, size=B)
                env.act_discrete(a)
                st.act(a)
            dense, cat = env.build_ahead_rows(n)
            dense, cat = dense.cpu().numpy().reshape(B, n, -1), cat.cpu().numpy().reshape(B, n, -1)
            for k in range(n):
                if k:
                    st.act(np.asarray(st.offline_action))
                _, d, c = st.features()
                assert np.array_equal(dense[:, k], d), (c0, n, k)
                assert np.array_equal(cat[:, k], c), (c0, n, k)
            env.check_error_flag()
            env.close()


@pytest.mark.parametrize('T', [9, 10])
def test_partition_copy_splits_envs_whose_logged_actions_part_later(tmp_path, T):
    """35 pairs of envs (2 i, 2 i + 1) with the same user and history whose logged slates agree up to step k = 1 + i % 8 and differ
    from there on, handed in as one class per pair behind act 0 (which both members take alike).  With n = 8 rows per env the rows of
    the acts 0 .. 7 are built: the second member stands for itself in the copy iff k <= 7, is appended to the copied active list and
    counted; k = 8 stays merged (no row shows step 8).  The rows themselves are the oracle's for both members."""
    import torch
    from rl4rs_amd import synth
    from rl4rs_amd.data import CatalogTables, RecordColumns
    from rl4rs_amd.device import DeviceEnv
    from oracle.state import OracleState
    pairs, n = 35, 8
    B = 2 * pairs
    cat_path = os.path.join(str(tmp_path), 'item_info.csv')
    cat_text = synth.make_catalog_text(seed=99)
    synth.write_text(cat_path, cat_text)
    base = synth.make_records(pairs, pages=2 if T > 9 else 1, seed=8, illegal_frac=0.0, special_ids=synth.special_ids_from_text(cat_text))
    records, ks = [], []
    for i, rec in enumerate(base):
        f = rec.split('@')
        k = 1 + i % 8
        slate = [int(x) for x in f[3].split(',')]
        twin = list(f)
        twin[3] = ','.join(str(x if j < k else x % 283 + 1) for j, x in enumerate(slate))
        records += [rec, '@'.join(twin)]
        ks.append(k)
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 100000, "seq_num": 2, "emb_size": 128, "page_items": 9, "hidden_units": 128, "max_steps": T,
           "action_emb_size": 32, "iteminfo_file": cat_path}
    cols = RecordColumns(records, cfg['maxlen'])
    env = DeviceEnv(cfg, CatalogTables(cat_path, 284, 32, False), False, cols.log_steps, True)
    env.load_batch(cols.exposed, cols.feedback, cols.history, cols.user_dense, cols.user_cat)
    env.reset()
    st = OracleState(cfg, records, seq=False)
    a = np.asarray(st.offline_action)
    assert np.array_equal(a[0::2], a[1::2])
    env.act_discrete(a)
    st.act(a)
    rep = torch.arange(B, dtype=torch.int32, device='cuda') // 2 * 2
    active = torch.arange(0, B, 2, dtype=torch.int32, device='cuda')
    cnt = torch.tensor([pairs], dtype=torch.int32, device='cuda')
    dense, cat, (rep_out, active_out, cnt_out) = env.build_ahead_rows(n, (rep, active, cnt))
    rep_out, active_out, cnt_out = rep_out.cpu().numpy(), active_out.cpu().numpy(), int(cnt_out.cpu()[0])
    split = [2 * i + 1 for i, k in enumerate(ks) if k <= n - 1]
    assert 0 < len(split) < pairs
    want_rep = np.arange(B) // 2 * 2
    want_rep[split] = split
    assert np.array_equal(rep_out, want_rep)
    assert cnt_out == pairs + len(split)
    assert np.array_equal(active_out[:pairs], np.arange(0, B, 2))
    assert sorted(active_out[pairs:cnt_out].tolist()) == split            # appended in no fixed order
    assert np.all(active_out[cnt_out:] == -1)                             # nothing behind the count is written
    assert np.array_equal(rep.cpu().numpy(), np.arange(B) // 2 * 2) and int(cnt.cpu()[0]) == pairs      # the act's own arrays stand
    dense, cat = dense.cpu().numpy().reshape(B, n, -1), cat.cpu().numpy().reshape(B, n, -1)
    for k in range(n):
        if k:
            st.act(np.asarray(st.offline_action))
        _, d, c = st.features()
        assert np.array_equal(dense[:, k], d) and np.array_equal(cat[:, k], c), k
        same = np.all(dense[0::2, k] == dense[1::2, k], axis=1) & np.all(cat[0::2, k] == cat[1::2, k], axis=1)
        assert np.array_equal(same, np.asarray(ks) > k), k                 # a pair's rows are equal exactly up to its step
    env.check_error_flag()
    env.close()
