#!/usr/bin/env python
"""The launches of a scorer forward, arm by arm: the check that a change to rl4rs_dien_forward issues what its parent issued.

    rocprofv3 --kernel-trace -d <dir> -o fl -- python tools/forward_launches.py run          (once per library: RL4RS_LIB=...)
    python tools/forward_launches.py compare <parent results.db> <this tree's results.db> [out.md]

`run` holds one scorer handle per arm of ARMS (every option that changes the form of a launch, alone, on top of the defaults) at
the smallest shapes that reach every form (L 16, 40 cache slots, inputs with duplicate row groups) and runs FORWARDS on each, then
one B = 64 Slate episode on device tensors and one through the reference-shaped API (mirror, fold, the carried partition through
the stepper).  It prints the arm and the forward it is about to run and puts one fill of MARK elements in front of each (the first
launch of the process is such a mark): `compare` cuts the two traces at the launches that look like the first one and compares,
segment by segment and stream by stream, the ordered list of (kernel, grid in workgroups, workgroup, LDS bytes).  A segment runs to
the next mark, so behind a forward's own launches it also holds the status read and whatever sets up the next forward."""
import os
import sqlite3
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CFG = {"maxlen": 16, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32}
SLOTS, ROWS, MARK = 40, 192, 7777
ARMS = [('default', 'fp16x2', '', {}), ('fp32', 'fp32', '', {})] + [(o, 'fp16x2', o, {}) for o in (
    'no_row_dedup', 'no_tier2_rows', 'no_augru_shadow', 'dup_store', 'dense_fork', 'no_gemm_group', 'no_dense_chain', 'no_gemm16',
    'din_v1', 'no_din16', 'augru_h16', 'cat_v1', 'no_cat_group', 'no_head_tables', 'no_head_fused', 'din_rows16')] + [
    ('cn24', 'fp16x2', '', {'category_feature_num': 24}), ('cn25', 'fp16x2', '', {'category_feature_num': 25}),
    ('u160', 'fp16x2', '', {'hidden_units': 160}),      # (hidden_units is a multiple of 32: 160 is the smallest the chain does not take)
    ('no_lazy_expand', 'fp16x2', 'no_lazy_expand', {})]  # (a tree from before DESIGN 31 does not know the name: its defaults then)
# (name, R, group, k_augru_x rows pin, distinct hint, row order, partition handed in)
FORWARDS = [('R96 g1 hint32', 96, 1, 0, 32, False, False), ('R96 g1', 96, 1, 0, 0, False, False),
            ('R192 g8 rows32', 192, 8, 32, 0, False, False), ('R192 g8 rows64', 192, 8, 64, 0, False, False),
            ('R189 g9 rows64', 189, 9, 64, 0, False, False), ('R96 g1 row order', 96, 1, 0, 0, True, False),
            ('R96 g1 partition', 96, 1, 0, 0, False, True)]


def _inputs(cfg, n_groups, group, rs):
    """row groups with duplicates, as tests/test_gpu_obs_step_launches.py::_groups: runs of one cache slot, templates repeated"""
    Cn, Dn = cfg['category_feature_num'], cfg['dense_feature_num']
    tpl = [(np.abs(rs.randn(group, Dn) * 3).astype(np.float32), rs.randint(0, 284, size=(group, Cn)).astype(np.int32)) for _ in range(5)]
    pick = rs.randint(0, 5, size=n_groups)
    run = np.sort(rs.randint(0, SLOTS, size=n_groups)).astype(np.int32)
    slots = np.stack([run, run % 2]).astype(np.int32)
    return slots, np.concatenate([tpl[i][0] for i in pick]), np.concatenate([tpl[i][1] for i in pick])


def _mark(torch, what):
    print(what, flush=True)
    torch.empty(MARK, dtype=torch.float32, device='cuda').fill_(0)


def _episode(torch, d, tensors):
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    text = synth.make_catalog_text(seed=4)
    synth.write_text(os.path.join(d, 'c.csv'), text)
    recs = synth.make_records(5, pages=1, seed=3, hash_size=2000, special_ids=synth.special_ids_from_text(text))
    synth.write_records(os.path.join(d, 'log.csv'), recs)
    cfg = dict(CFG, maxlen=64, batch_size=64, category_hash_size=2000, sample_file=os.path.join(d, 'log.csv'),
               iteminfo_file=os.path.join(d, 'c.csv'), cache_size=5, model_seed=3, scorer_precision='fp16x2',
               scorer_kernels='augru_rows64')      # (the pin: a batch this small folds its reward step too)
    if tensors:
        cfg['return_tensors'] = True
    np.random.seed(7)
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(11)
    torch.cuda.synchronize()
    _mark(torch, 'episode B64 %s' % ('device tensors' if tensors else 'reference-shaped'))
    env.reset()
    for _ in range(9):
        env.step(env.offline_action)
    torch.cuda.synchronize()


def run():
    import torch
    from rl4rs_amd.device import DeviceDien, DIEN_N_ACTIVE, DIEN_ROW_REP, DIEN_ROW_ACTIVE
    from rl4rs_amd.nets.dien import init_dien_weights
    _mark(torch, 'start')
    for arm, precision, kernels, over in ARMS:
        cfg = dict(CFG, scorer_precision=precision, scorer_kernels=kernels, **over)
        rs = np.random.RandomState(3)
        try:
            net = DeviceDien(cfg, init_dien_weights(cfg, seed=9, emb_scale=0.5, bias_noise=0.2), max_rows=ROWS, max_slots=SLOTS)
        except (KeyError, ValueError):
            if kernels != 'no_lazy_expand':
                raise
            net = DeviceDien(dict(cfg, scorer_kernels=''), init_dien_weights(cfg, seed=9, emb_scale=0.5, bias_noise=0.2), max_rows=ROWS, max_slots=SLOTS)
        seq = rs.randint(1, 284, size=(SLOTS, 2, 16)).astype(np.int32)
        seq[::2, 1, :] = 0
        for s in range(2):
            net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
        takes = precision == 'fp16x2' and not (set(kernels.split(',')) & {'no_row_dedup', 'dup_store', 'augru_h16', 'din_v1', 'no_din16'})
        for what, R, group, rows, hint, order, part in FORWARDS:
            if part and not takes:
                continue                                    # this arm's forward takes no partition (an error by contract)
            slots, dense, cat = _inputs(cfg, R // group, group, rs)
            sl, dn, ct = torch.from_numpy(slots).cuda(), torch.from_numpy(dense).cuda(), torch.from_numpy(cat).cuda()
            net.set_augru_rows(rows)
            net.set_distinct_hint(hint)
            net.set_row_order(torch.from_numpy(rs.permutation(R // group).astype(np.int32)).cuda() if order else None)
            held = None
            if part:                                        # the partition a content forward found, handed back in
                net.forward(R, group, dn, ct, sl, True, True)
                held = [net.snapshot(w, R)[:n].contiguous() for w, n in ((DIEN_ROW_REP, R // group), (DIEN_ROW_ACTIVE, R // group), (DIEN_N_ACTIVE, 1))]
            torch.cuda.synchronize()
            _mark(torch, '%s: %s' % (arm, what))
            if held:
                net.set_row_partition(*held)
            net.forward(R, group, dn, ct, sl, True, True)
            net.check_status()
        net.close()
    with tempfile.TemporaryDirectory() as d:
        for sub, tensors in (('a', True), ('b', False)):
            os.makedirs(os.path.join(d, sub))
            _episode(torch, os.path.join(d, sub), tensors)
    _mark(torch, 'end')


def _labels():
    out = ['start']
    for arm, precision, kernels, _ in ARMS:
        takes = precision == 'fp16x2' and not (set(kernels.split(',')) & {'no_row_dedup', 'dup_store', 'augru_h16', 'din_v1', 'no_din16'})
        out += ['%s: %s' % (arm, f[0]) for f in FORWARDS if takes or not f[6]]
    return out + ['episode B64 device tensors', 'episode B64 reference-shaped', 'end']


def _segments(path):
    """-> [[(stream, kernel, grid, workgroup, lds)] per segment]; a segment starts at every launch shaped like the trace's first"""
    db = sqlite3.connect(path)
    cols = [r[1] for r in db.execute("pragma table_info('kernels')")]
    pick = lambda *names: next(n for n in names if n in cols)
    st = pick('start', 'start_timestamp')
    stream = pick('stream_id', 'stream', 'queue_id', 'queue')
    lds = pick('lds_size', 'lds_block_size', 'group_segment_size', 'lds')
    q = "select name, %s, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z, %s from kernels order by %s" % (stream, lds, st)
    segs, mark = [], None
    for name, sid, gx, gy, gz, wx, wy, wz, l in db.execute(q):
        mark = mark or (name, gx, wx)
        if (name, gx, wx) == mark:
            segs.append([])
        else:
            segs[-1].append((sid, name, '%dx%dx%d' % (gx // max(wx, 1), gy // max(wy, 1), gz // max(wz, 1)), '%dx%dx%d' % (wx, wy, wz), int(l)))
    return segs


def _per_stream(seg):
    streams = []
    for e in seg:
        if e[0] not in streams:
            streams.append(e[0])
    return [[e[1:] for e in seg if e[0] == s] for s in streams]        # stream ids differ between processes: order of first use


def compare(a_path, b_path, out):
    a, b, labels = _segments(a_path), _segments(b_path), _labels()
    lines = ['# Launches of the scorer forward: parent library against this tree (`tools/forward_launches.py`)', '',
             'segments: parent %d, this tree %d, expected %d' % (len(a), len(b), len(labels)), '']
    same_all = len(a) == len(b) == len(labels)
    for i, lab in enumerate(labels[:min(len(a), len(b))]):
        pa, pb = _per_stream(a[i]), _per_stream(b[i])
        same = pa == pb
        same_all = same_all and same and (lab in ('start', 'end') or len(a[i]) > 0)
        lines.append('## %s - %s (%d launches)' % (lab, 'identical' if same else 'DIFFERENT', len(a[i])))
        for k, (sa, sb) in enumerate(zip(pa, pb) if not same else zip(pa, pa)):
            for tag, s in (('parent', sa),) + ((('this tree', sb),) if not same else ()):
                lines.append('- stream %d, %s: ' % (k, tag) + ' -> '.join('`%s` %s/%s lds %d' % (n.replace('void ', '').split('(')[0][:48], g, w, l) for n, g, w, l in s))
        lines.append('')
    lines.insert(3, 'RESULT: %s' % ('every segment identical' if same_all else 'DIFFERENT'))
    text = '\n'.join(lines) + '\n'
    if out:
        open(out, 'w').write(text)
    print(text if len(text) < 4000 else '\n'.join(lines[:4]))
    return 0 if same_all else 1


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run()
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else None))
