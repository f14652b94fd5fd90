#!/usr/bin/env python
"""Speed of the on-device Exact-K (one GPU).

  update   the generator update (rl4rs_exactk_loss_grad + rl4rs_exactk_adam_step: teacher-forced forward, loss, full backward, Adam)
           at N = 256 and N = 4096 on the reference's net (A = 284, H = 64, 4 heads, 2 blocks, dropout 0.1) against the SAME pass
           written in eager torch on the GPU (matmul autograd, torch's own dropout at the two sites, torch.optim.Adam).  The two
           alternate in one process, ``--pairs`` pairs, every sample = ``--updates`` updates between two synchronisations.
  decode   the sampled and the greedy decode (rl4rs_exactk_decode) at the same sizes against the eager-torch decoder
           (torch.multinomial / argmax per step), the same way.
  beam     beam search (rl4rs_exactk_decode_beam, B = 3) at the same sizes against the greedy decode of N rows on the same handle (the
           price of beam search over greedy) and against the greedy decode of 3 N rows (what 3 N replicated decoder rows would cost
           with the encoder run for each; one call where max_rows allows, otherwise chunks of N rows), the same way.
  loop     SlateRecEnv-v0 B = 4096 env-steps/s with ExactKTrainer in the loop (two climbs of 9 steps per iteration).

One JSON line on stdout (and --out FILE).  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OD, A, H, HEADS, BLOCKS, VOCAB, RATE, T = 256, 284, 64, 4, 2, 500, 0.1, 9
PAD = -4294967295.0


class TorchExactK(object):
    """The yardstick: the same generator in eager torch."""

    def __init__(self, flat, loc, special):
        import torch
        from rl4rs_amd.nets.exactk import split
        self.t = torch
        f = torch.from_numpy(flat).cuda()
        self.names = list(split(f, OD, H, BLOCKS, VOCAB).keys())
        self.p = dict((k, v.clone().requires_grad_(True)) for k, v in split(f, OD, H, BLOCKS, VOCAB).items())
        self.opt = torch.optim.Adam(list(self.p.values()), lr=1e-3, betas=(0.9, 0.98), eps=1e-8)
        self.loc = torch.from_numpy(loc.astype(bool)).cuda()
        self.special = torch.from_numpy(special.astype(bool)).cuda()

    def _ln(self, x, g, b):
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        return g * ((x - mean) / (var + 1e-8) ** 0.5) + b

    def encode(self, obs):
        t, p = self.t, self.p
        N, D, dh = obs.shape[0], 2 * H, 2 * H // HEADS
        eu = t.relu(obs @ p['user_W'] + p['user_b'])
        x = t.cat([eu[:, None, :].expand(N, A, H), (p['table'][:A] * H ** 0.5)[None].expand(N, A, H)], dim=2)
        x = t.nn.functional.dropout(x, RATE, True)
        for b in range(BLOCKS):
            g = lambda n: p['blk%d_%s' % (b, n)]
            heads = lambda y: y.reshape(N, A, HEADS, dh).permute(0, 2, 1, 3)
            Q, K, V = (heads(t.relu(x @ g('W' + c) + g('b' + c))) for c in 'qkv')
            live = x.detach().sum(-1) != 0
            s = t.where(live[:, None, None, :], Q @ K.transpose(2, 3) / dh ** 0.5, t.full((), PAD, device='cuda'))
            pr = t.nn.functional.dropout(t.softmax(s, dim=-1) * live[:, None, :, None], RATE, True)
            y = self._ln((pr @ V).permute(0, 2, 1, 3).reshape(N, A, D) + x, g('ln1_g'), g('ln1_b'))
            x = self._ln(t.relu(y @ g('W1') + g('b1')) @ g('W2') + g('b2') + y, g('ln2_g'), g('ln2_b'))
        return x

    def _att(self, k, ref, query, dec):
        p, t = self.p, self.t
        return (p[k + '_v'] * t.tanh(ref + (query @ p[k + '_Wq'])[:, None] + (dec @ p[k + '_Wdec'])[:, None] + p[k + '_bias'])).sum(-1)

    def decoder(self, enc, path=None, greedy=False):
        t, p = self.t, self.p
        N, D = enc.shape[0], 2 * H
        ref_g, ref_p = enc @ p['glimpse_Wref'], enc @ p['pointer_Wref']
        c, h = p['init_c'][None].expand(N, D), p['init_h'][None].expand(N, D)
        rows = t.arange(N, device='cuda')
        picked = t.zeros((N, A), dtype=t.bool, device='cuda')
        outs, logits, picks = [], [], []
        for s in range(T):
            x = p['first_input'][None].expand(N, D) if s == 0 else enc[rows, picks[-1]]
            i, j, f, o = (t.cat([x, h], dim=1) @ p['lstm_W'] + p['lstm_b']).split(D, dim=1)
            c = t.sigmoid(f + 1.0) * c + t.sigmoid(i) * t.tanh(j)
            h = t.sigmoid(o) * t.tanh(c)
            if s == 0:
                intra = t.zeros_like(h)
            elif s == 1:
                intra = outs[0]
            else:
                bef = t.stack(outs, dim=1)
                sc = (p['intra_v'] * t.tanh(bef @ p['intra_Wbef'] + (h @ p['intra_Wb'])[:, None] + p['intra_bias'])).sum(-1)
                intra = (t.softmax(sc, dim=1)[:, :, None] * bef).sum(1)
            outs.append(h)
            q = (t.softmax(self._att('glimpse', ref_g, h, intra), dim=1)[:, :, None] * enc).sum(1)
            sc = self._att('pointer', ref_p, q, intra)
            any_sp = (picked & self.special[None]).any(dim=1)
            ok = self.loc[s // 3][None] & ~picked & ~(any_sp[:, None] & self.special[None])
            lg = t.where(ok, sc, t.full((), PAD, device='cuda'))
            logits.append(lg)
            if path is not None:
                a = path[:, s]
            elif greedy:
                a = lg.argmax(dim=1)
            else:
                a = t.multinomial(t.softmax(lg, dim=1), 1)[:, 0]
            picks.append(a)
            picked = picked.clone()
            picked[rows, a] = True
        return t.stack(logits, dim=1), t.stack(picks, dim=1)

    def update(self, obs, path, w):
        t = self.t
        logits, _ = self.decoder(self.encode(obs), path=path)
        ce = t.logsumexp(logits, dim=2) - logits.gather(2, path[:, :, None])[:, :, 0]
        loss = (w * ce.sum(1)).mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()

    def decode(self, obs, greedy):
        with self.t.no_grad():
            return self.decoder(self.encode(obs), greedy=greedy)[1]


def timed(fn, updates):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(updates):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / updates


def paired(hip, tor, pairs, updates):
    for _ in range(3):                                    # warm-up: code objects, allocator, autograd graph caches
        hip()
        tor()
    ps = [(timed(hip, updates) * 1e6, timed(tor, updates) * 1e6) for _ in range(pairs)]
    h, t = np.array([p[0] for p in ps]), np.array([p[1] for p in ps])
    return dict(unit='us per call', pairs=[[round(a, 1), round(b, 1)] for a, b in ps], hip_median=round(float(np.median(h)), 1),
                torch_median=round(float(np.median(t)), 1), ratio_torch_over_hip=round(float(np.median(t) / np.median(h)), 2),
                hip_faster_in_every_pair=bool((h < t).all()))


def net_legs(args, N):
    import torch
    from rl4rs_amd import synth
    from rl4rs_amd.data import CatalogTables
    from rl4rs_amd.device import DeviceExactK
    from rl4rs_amd.nets.exactk import init_exactk_params
    d = tempfile.mkdtemp(prefix='exactk_rate_')
    synth.write_text(os.path.join(d, 'item_info.csv'), synth.make_catalog_text(seed=1234))
    cat = CatalogTables(os.path.join(d, 'item_info.csv'), A)
    rs = np.random.RandomState(0)
    flat = init_exactk_params(OD, H, BLOCKS, VOCAB, seed=1)
    net = DeviceExactK(cat.location_mask[:3], cat.is_special, max_rows=N, obs_dim=OD, action_size=A, hidden_units=H, num_heads=HEADS,
                       num_blocks=BLOCKS, vocab=VOCAB, dropout_rate=RATE, params=flat)
    ref = TorchExactK(flat, np.asarray(cat.location_mask[:3]), np.asarray(cat.is_special))
    obs = torch.from_numpy(rs.randn(N, OD).astype(np.float32)).cuda()
    w = torch.from_numpy(rs.randn(N).astype(np.float32)).cuda()
    path, _ = net.decode(obs, greedy=False, seed=1, step=0)
    path64 = path.to(torch.int64)
    step = [0]

    def hip_update():
        step[0] += 1
        net.loss_grad(obs, path, w, seed=1, step=step[0])
        net.adam_step(lr=1e-3)

    def hip_decode(greedy):
        step[0] += 1
        net.decode(obs, greedy=greedy, seed=1, step=step[0], out=path)

    out = dict(rows=N, updates_per_sample=args.updates)
    out['update'] = paired(hip_update, lambda: ref.update(obs, path64, w), args.pairs, args.updates)
    out['decode_sample'] = paired(lambda: hip_decode(False), lambda: ref.decode(obs, False), args.pairs, args.updates)
    out['decode_greedy'] = paired(lambda: hip_decode(True), lambda: ref.decode(obs, True), args.pairs, args.updates)
    net.close()
    return out


def paired_ab(a, b, name_a, name_b, pairs, updates):
    """``paired`` for two device paths: alternating samples of a and b"""
    for _ in range(3):
        a()
        b()
    ps = [(timed(a, updates) * 1e6, timed(b, updates) * 1e6) for _ in range(pairs)]
    x, y = np.array([p[0] for p in ps]), np.array([p[1] for p in ps])
    return {'unit': 'us per call', 'pairs': [[round(u, 1), round(v, 1)] for u, v in ps], name_a + '_median': round(float(np.median(x)), 1),
            name_b + '_median': round(float(np.median(y)), 1),
            'ratio_%s_over_%s' % (name_a, name_b): round(float(np.median(x) / np.median(y)), 2)}


def beam_legs(args, N, B=3):
    import torch
    from rl4rs_amd import synth
    from rl4rs_amd.data import CatalogTables
    from rl4rs_amd.device import DeviceExactK
    from rl4rs_amd.nets.exactk import init_exactk_params
    d = tempfile.mkdtemp(prefix='exactk_rate_')
    synth.write_text(os.path.join(d, 'item_info.csv'), synth.make_catalog_text(seed=1234))
    cat = CatalogTables(os.path.join(d, 'item_info.csv'), A)
    rs = np.random.RandomState(0)
    rows = B * N if B * N <= 1024 else N                   # the handle's max_rows: 3 N rows in one call where that stays small
    net = DeviceExactK(cat.location_mask[:3], cat.is_special, max_rows=rows, obs_dim=OD, action_size=A, hidden_units=H, num_heads=HEADS,
                       num_blocks=BLOCKS, vocab=VOCAB, dropout_rate=RATE, params=init_exactk_params(OD, H, BLOCKS, VOCAB, seed=1))
    obs3 = torch.from_numpy(rs.randn(B * N, OD).astype(np.float32)).cuda()
    obs = obs3[:N].contiguous()
    chunks = [obs3[i:i + rows].contiguous() for i in range(0, B * N, rows)]
    path = torch.empty((rows, T), dtype=torch.int32, device='cuda')
    step = [0]

    def beam():
        step[0] += 1
        net.decode_beam(obs, beam_size=B, seed=1, step=step[0])

    def greedy():
        step[0] += 1
        net.decode(obs, greedy=True, seed=1, step=step[0], out=path[:N])

    def greedy_replicated():
        step[0] += 1
        for c in chunks:
            net.decode(c, greedy=True, seed=1, step=step[0], out=path[:c.shape[0]])

    out = dict(rows=N, beam=B, updates_per_sample=args.updates, replicated_rows=B * N, replicated_calls=len(chunks))
    out['beam_vs_greedy'] = paired_ab(beam, greedy, 'beam', 'greedy', args.pairs, args.updates)
    out['beam_vs_replicated_greedy'] = paired_ab(beam, greedy_replicated, 'beam', 'replicated', args.pairs, args.updates)
    net.close()
    return out


def loop_leg(args, steps=3):
    import torch
    import rl4rs_amd
    from rl4rs_amd import synth
    from rl4rs_amd.env.slate import SlateRecEnv, SlateState
    from rl4rs_amd.train import ExactKTrainer
    B = args.batch
    d = tempfile.mkdtemp(prefix='exactk_rate_')
    text = synth.make_catalog_text(seed=1234)
    synth.write_text(os.path.join(d, 'item_info.csv'), text)
    synth.write_records(os.path.join(d, 'log.csv'), synth.make_records(8193, seed=1000, illegal_frac=0.05,
                                                                       special_ids=synth.special_ids_from_text(text)))
    cfg = {"maxlen": 64, "batch_size": B, "action_size": 284, "class_num": 2, "dense_feature_num": 432, "category_feature_num": 21,
           "category_hash_size": 100000, "seq_num": 2, "emb_size": 128, "page_items": 9, "hidden_units": 128, "max_steps": T,
           "action_emb_size": 32, "sample_file": os.path.join(d, 'log.csv'), "iteminfo_file": os.path.join(d, 'item_info.csv'),
           "is_eval": False, "cache_size": 2048, "model_seed": 7, "return_tensors": True}
    env = rl4rs_amd.make('SlateRecEnv-v0', recsim=SlateRecEnv(cfg, state_cls=SlateState))
    env.seed(1000)
    env.sim._recData.store.preload(torch.device('cuda', torch.cuda.current_device()))
    tr = ExactKTrainer(env, seed=1000)
    tr.train_iteration()
    tr.train_iteration()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.train_iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_steps = B * T * tr.samples * steps
    tr.close()
    return dict(value=round(n_steps / dt, 1), unit='env-steps/s', ms_per_iteration=round(dt / steps * 1e3, 3),
                workload='SlateRecEnv-v0 B=%d T=%d, 2 sampled decodes + 2 x 9 env steps + critic and generator updates' % (B, T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='net,beam,loop')
    ap.add_argument('--rows', default='256,4096')
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--updates', type=int, default=5)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'exactk_rate.py measures on the GPU only'
    result = dict(tool='exactk_rate', device=torch.cuda.get_device_name(0), torch=torch.__version__,
                  command='python tools/exactk_rate.py ' + ' '.join(sys.argv[1:]))
    legs = args.legs.split(',')
    if 'net' in legs:
        result['net'] = [net_legs(args, int(n)) for n in args.rows.split(',')]
    if 'beam' in legs:
        result['beam'] = [beam_legs(args, int(n)) for n in args.rows.split(',')]
    if 'loop' in legs:
        result['loop'] = loop_leg(args)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
