#!/usr/bin/env python
"""Timing experiment (library built with -DRL4RS_H16_TRACE): s_memtime marks of workgroup (0,0), steps 8..11, per wave.  Prints the
per-segment cycle counts.

    python tools/h16_trace.py [R]                          k_augru_h16 (scorer_kernels='augru_h16' era; the forward's AUGRU launch)
        marks: 0 step start | 1 slot R done | 2 slot U done | 3 after barrier | 4 slot C done | 5 E2 done | 6 after barrier
    python tools/h16_trace.py --gru [R] [--kernels gru_h16_v1]     the first GRU of an encode of R distinct histories:
        k_gru_h16r, waves 0..3 (rc role): slot R | reset gate | wait barrier 1 | slot C | blend | wait barrier 2
                    waves 4..7 (u role):  slot U | update gate | stores | wait barrier 1 | stagings + gathers | wait barrier 2
        k_gru_h16 (gru_h16_v1), waves 0..3: slot R | slot U + reset gate | wait barrier 1 | slot C + update gate | blend + stores | wait barrier 2
    and, like tools/x_trace.py, the mean of steps 8..10 per role."""
import argparse
import os
import sys
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('R', nargs='?', type=int, default=4096)
ap.add_argument('--gru', action='store_true')
ap.add_argument('--kernels', default='')
args = ap.parse_args()
DUMP = '/tmp/h16_trace.bin'
os.environ['RL4RS_GRU_TRACE_DUMP' if args.gru else 'RL4RS_H16_TRACE_DUMP'] = DUMP
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl4rs_amd.nets.dien import init_dien_weights
from rl4rs_amd.device import DeviceDien

CFG = {"maxlen": 64, "batch_size": 8, "action_size": 284, "class_num": 2, "dense_feature_num": 432,
       "category_feature_num": 21, "category_hash_size": 3000, "seq_num": 2, "emb_size": 128,
       "page_items": 9, "hidden_units": 128, "max_steps": 9, "action_emb_size": 32, "scorer_precision": "fp16x2",
       "scorer_kernels": args.kernels}
R = args.R
w = init_dien_weights(CFG, seed=3)
rs = np.random.RandomState(0)
net = DeviceDien(CFG, w, max_rows=R, max_slots=R)
seq = rs.randint(1 if args.gru else 0, 284, size=(R, 2, 64)).astype(np.int32)          # --gru: no zero prefix, all 64 steps computed
for _ in range(3 if args.gru else 1):      # the dump at launch k holds the marks of launch k-1
    for s in range(2):
        net.encode(s, torch.from_numpy(np.ascontiguousarray(seq[:, s])).cuda(), 0)
if not args.gru:
    slots = torch.arange(R, dtype=torch.int32).repeat(2, 1).contiguous().cuda()
    dense = torch.from_numpy(np.abs(rs.randn(R, 432)).astype(np.float32)).cuda()
    cat = torch.from_numpy(rs.randint(0, 284, size=(R, 21)).astype(np.int32)).cuda()
    for _ in range(3):
        net.forward(R, 1, dense, cat, slots, want_obs=True, want_prob=False)
torch.cuda.synchronize()
tr = np.fromfile(DUMP, dtype=np.uint64).reshape(8, 4, 8).astype(np.int64)
if not args.gru:
    roles = {'all': (range(8), ['slotR', 'slotU', 'bar1', 'slotC', 'E2', 'bar2', 'next'])}
elif 'gru_h16_v1' in args.kernels:
    roles = {'v1': (range(4), ['slotR', 'slotU+r', 'bar1', 'slotC+u', 'blend+st', 'bar2', 'next'])}
else:
    roles = {'rc': (range(4), ['slotR', 'rgate', 'bar1', 'slotC', 'blend', 'bar2', 'next']),
             'u': (range(4, 8), ['slotU', 'ugate', 'stores', 'bar1', 'stage+gather', 'bar2', 'next'])}
for role, (waves, names) in roles.items():
    segs = []
    for wv in waves:
        for st in range(3):
            m = tr[wv, st]
            seg = [m[k + 1] - m[k] for k in range(6)] + [tr[wv, st + 1, 0] - m[6]]
            segs.append(seg + [tr[wv, st + 1, 0] - m[0]])
            print('%s wave %d step %d: ' % (role, wv, st + 8) + '  '.join('%s %5d' % (n, v) for n, v in zip(names, seg)) +
                  '   total %d' % (tr[wv, st + 1, 0] - m[0]))
    mean = np.mean(np.array(segs), axis=0)
    print('%s MEAN steps 8..10: ' % role + '  '.join('%s %.0f' % (n, v) for n, v in zip(names + ['total'], mean)))
