#!/usr/bin/env python
"""Time of one OPE step of a mask-model policy (one GPU), both ``q_mode``s.

  step      ``OpeLog.record_step`` (rl4rs_policy_ope_step: two GEMMs and ONE row launch that writes pi[t], q[t] and the action)
  composed  what the same step was composed of before: ``DevicePolicy.greedy(want_q=True)`` + ``OpeLog.record_policy(logits=True)`` +
            ``OpeLog.record_q`` (the masked [B, A] row written once and read twice more); for ``q_mode`` 0 also the handle's
            ``evaluate`` for the value head and a ``record_column``: that is what 'vf_preds' cost without the fused step.

B = 2048 (the driver's eval batch), A = 284, a 256 -> 64 -> 284 handle.  Both sides must agree on action, pi and q before anything
is timed (pi to rtol 1e-12: the same float64 rule on the same float32 row; q_mode 0's value to 2e-5 abs: another kernel's forward).
The two alternate in one process: ``--pairs`` pairs, every sample = ``--calls`` calls between two device events, after a warm-up
of both.  One JSON line on stdout (and --out FILE) with the per-call medians, the ratio per pair and its spread.  Needs a GPU: there
is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, OD, HID, A = 2048, 256, 64, 284


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=7)
    ap.add_argument('--calls', type=int, default=300)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.pairs < 5 or args.calls < 200:
        ap.error('at least 5 pairs of at least 200 calls')
    import torch
    from rl4rs_amd.device import DevicePolicy
    from rl4rs_amd.ope import OpeLog
    assert torch.cuda.is_available(), 'ope_step_rate needs a GPU'
    rs = np.random.RandomState(0)
    pol = DevicePolicy(OD, HID, A, max_rows=B, seed=1)
    obs = torch.from_numpy(rs.randn(B, OD).astype(np.float32)).cuda()
    mask = rs.rand(B, A) < 0.4
    mask[np.arange(B), rs.randint(0, A, size=B)] = True
    words = np.zeros((B, (A + 31) // 32), dtype=np.uint32)
    for k in range(A):
        words[:, k >> 5] |= mask[:, k].astype(np.uint32) << np.uint32(k & 31)
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    logged = torch.from_numpy(rs.randint(0, A, size=B).astype(np.int32)).cuda()
    log = OpeLog(B, 2)
    log.begin(B, 2)
    act = torch.empty(B, dtype=torch.int32, device='cuda')

    def step(q_mode):
        return log.record_step(0, pol, obs, bits, logged, q_mode, actions_out=act)

    def composed(q_mode):
        a, row = pol.greedy(obs, bits, want_q=True, out=act)
        log.record_policy(1, row, logged, logits=True)
        if q_mode:
            log.record_q(1, row, a)
        else:
            log.record_column(1, 'q', pol.evaluate(obs, a, bits)[1])
        return a

    def timed(fn, q_mode):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.calls):
            fn(q_mode)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / args.calls             # microseconds per call

    result = {'B': B, 'obs_dim': OD, 'hidden': HID, 'action_size': A, 'pairs': args.pairs, 'calls': args.calls}
    for q_mode in (1, 0):
        a_s = step(q_mode).clone()
        a_c = composed(q_mode).clone()
        pi, q = log.column('pi').cpu().numpy(), log.column('q').cpu().numpy()
        assert torch.equal(a_s, a_c), 'the two sides disagree on the action'
        assert np.allclose(pi[0], pi[1], rtol=1e-12, atol=0), 'the two sides disagree on pi'
        assert np.array_equal(q[0], q[1]) if q_mode else np.abs(q[0] - q[1]).max() < 2e-5, 'the two sides disagree on q'
        for fn in (step, composed):                                    # warm-up of both
            timed(fn, q_mode)
        t_step, t_comp = [], []
        for _ in range(args.pairs):
            t_step.append(timed(step, q_mode))
            t_comp.append(timed(composed, q_mode))
        ratio = np.array(t_comp) / np.array(t_step)
        result['q_mode_%d' % q_mode] = {'step_us': float(np.median(t_step)), 'composed_us': float(np.median(t_comp)),
                                        'step_us_all': [round(v, 2) for v in t_step], 'composed_us_all': [round(v, 2) for v in t_comp],
                                        'composed_over_step': float(np.median(ratio)), 'ratio_min': float(ratio.min()),
                                        'ratio_max': float(ratio.max())}
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
