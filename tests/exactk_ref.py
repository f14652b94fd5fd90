"""float64 restatement of the on-device Exact-K (include/rl4rs_hip.h, "On-device Exact-K"): the attention encoder, the LSTM pointer
decoder with its allowed-set rule, the dropout masks of the counter hash, the weighted cross-entropy loss with its gradient (torch
autograd on the CPU), the critic and TF-form Adam.

Test infrastructure only.  PARITY UNPINNED: TensorFlow 1.15 is absent, so this restates rl4rs/nets/exact_k/{model,layers,modules}.py
as the reference's defaults configure them; tests/test_exactk_host.py checks the gradient below against central finite differences.

``fp32_yardstick`` runs the same restatement in float32 eager torch on the CPU against float64 on the very inputs of a case: the
GPU tests' bars are BAR_FACTOR x that measured error (MEASURED), never a number taken from the code under test."""
import numpy as np
import torch

import td3_ref
from rl4rs_amd.nets import exactk as NX

PAD = -4294967295.0            # -2^32 + 1
PAD32 = float(np.float32(PAD))  # what float32 holds for it: -2^32 (the device's and the fp32 yardstick's padding value)
T = 9
BAR_FACTOR = 4.0


class Dims(object):
    def __init__(self, A=284, H=64, heads=4, blocks=2, vocab=None, od=256, rate=0.0):
        self.A, self.H, self.heads, self.blocks, self.od = int(A), int(H), int(heads), int(blocks), int(od)
        self.vocab = int(vocab if vocab is not None else A + 3)
        self.D, self.rate = 2 * self.H, float(rate)

    def names(self):
        return [n for n, _, _ in NX.shapes(self.od, self.H, self.blocks, self.vocab)]

    def split(self, flat):
        return NX.split(flat, self.od, self.H, self.blocks, self.vocab)

    def n_params(self):
        return NX.param_count(self.od, self.H, self.blocks, self.vocab)


# ---- dropout masks -------------------------------------------------------------------------------------------------------
def keep(rate, seed, step, site, rows, cols):
    """Keep factors 0 or 1 / (1 - rate) of the elements (rows x cols broadcast): u(seed, step, row, site * 65536 + col) >= rate."""
    rows, cols = np.asarray(rows, dtype=np.uint64), np.asarray(cols, dtype=np.uint64)
    if rate <= 0:
        return np.ones(np.broadcast(rows, cols).shape)
    u = td3_ref.uniform01(seed, step, rows, np.uint64(site * 65536) + cols).astype(np.float32)
    return np.where(u >= np.float32(rate), 1.0 / (1.0 - float(np.float32(rate))), 0.0)


def enc_keep(dm, N, seed, step, pas):
    rows = np.arange(N * dm.A, dtype=np.uint64).reshape(N, dm.A, 1)
    return keep(dm.rate, seed, step, 32 * pas, rows, np.arange(dm.D, dtype=np.uint64).reshape(1, 1, dm.D))


def attn_keep(dm, N, seed, step, pas, block):
    """[N, heads, A(query), A(key)]"""
    rows = np.arange(N * dm.heads * dm.A, dtype=np.uint64).reshape(N, dm.heads, dm.A, 1)
    return keep(dm.rate, seed, step, 32 * pas + 1 + block, rows, np.arange(dm.A, dtype=np.uint64).reshape(1, 1, 1, dm.A))


# ---- allowed sets --------------------------------------------------------------------------------------------------------
def allowed_sets(path, loc, special):
    """bool [N, 9, A]: not yet picked, in location_mask[t // 3], no special item once a special item has been picked."""
    path = np.asarray(path)
    N, A = len(path), loc.shape[1]
    out = np.zeros((N, T, A), dtype=bool)
    picked = np.zeros((N, A), dtype=bool)
    rows = np.arange(N)
    for t in range(T):
        any_special = (picked & special[None, :]).any(axis=1)
        out[:, t] = loc[t // 3][None, :] & ~picked & ~(any_special[:, None] & special[None, :])
        picked[rows, path[:, t]] = True
    return out


def random_slates(N, loc, special, rs):
    """N random valid slates under the rule."""
    A = loc.shape[1]
    path = np.zeros((N, T), dtype=np.int32)
    for n in range(N):
        picked = np.zeros(A, dtype=bool)
        for t in range(T):
            ok = loc[t // 3] & ~picked & ~((picked & special).any() & special)
            path[n, t] = rs.choice(np.nonzero(ok)[0])
            picked[path[n, t]] = True
    return path


# ---- generator -----------------------------------------------------------------------------------------------------------
def _ln(x, g, b):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return g * ((x - mean) / (var + 1e-8) ** 0.5) + b


RELU_TAP = None                # relu_sites() sets it: called with (pre-activation, output) at every relu of encode()


def _relu(z):
    o = torch.relu(z)
    if RELU_TAP is not None:
        RELU_TAP(z, o)
    return o


def encode(p, obs, dm, seed=0, step=0, pas=0):
    """enc [N, A, D] from the parameter dict p (torch tensors of one dtype)."""
    dt = obs.dtype
    N, A, H, D, hd = obs.shape[0], dm.A, dm.H, dm.D, dm.heads
    eu = _relu(obs @ p['user_W'] + p['user_b'])
    item = p['table'][:A] * (H ** 0.5)
    x = torch.cat([eu[:, None, :].expand(N, A, H), item[None].expand(N, A, H)], dim=2)
    x = x * torch.from_numpy(enc_keep(dm, N, seed, step, pas)).to(dt)
    dh = D // hd
    for b in range(dm.blocks):
        g = lambda n: p['blk%d_%s' % (b, n)]
        Q = _relu(x @ g('Wq') + g('bq')).reshape(N, A, hd, dh).permute(0, 2, 1, 3)
        K = _relu(x @ g('Wk') + g('bk')).reshape(N, A, hd, dh).permute(0, 2, 1, 3)
        V = _relu(x @ g('Wv') + g('bv')).reshape(N, A, hd, dh).permute(0, 2, 1, 3)
        s = Q @ K.transpose(2, 3) / (dh ** 0.5)
        live = (x.detach().sum(-1) != 0)                       # [N, A]: key and query masks
        s = torch.where(live[:, None, None, :], s, torch.full_like(s, PAD))
        pr = torch.softmax(s, dim=-1) * live[:, None, :, None].to(dt)
        pr = pr * torch.from_numpy(attn_keep(dm, N, seed, step, pas, b)).to(dt)
        o = (pr @ V).permute(0, 2, 1, 3).reshape(N, A, D)
        y = _ln(o + x, g('ln1_g'), g('ln1_b'))
        f = _relu(y @ g('W1') + g('b1')) @ g('W2') + g('b2')
        x = _ln(f + y, g('ln2_g'), g('ln2_b'))
    return x


def _attention(p, k, enc_ref, query, dec_ref):
    return (p[k + '_v'] * torch.tanh(enc_ref + (query @ p[k + '_Wq'])[:, None, :] + (dec_ref @ p[k + '_Wdec'])[:, None, :]
                                     + p[k + '_bias'])).sum(-1)


def run_decoder(p, enc, dm, loc, special, path=None, chooser=None):
    """The decoder along a given path (teacher-forced) or along the picks of chooser(t, logits_t [N, A] numpy float64) -> int [N].
    -> (logits [N, 9, A], path [N, 9])"""
    N, D, A = enc.shape[0], dm.D, dm.A
    ref_g, ref_p = enc @ p['glimpse_Wref'], enc @ p['pointer_Wref']
    c, h = p['init_c'][None].expand(N, D), p['init_h'][None].expand(N, D)
    outs, logits = [], []
    rows = torch.arange(N)
    picked = np.zeros((N, A), dtype=bool)
    out_path = np.zeros((N, T), dtype=np.int32)
    for t in range(T):
        x = p['first_input'][None].expand(N, D) if t == 0 else enc[rows, torch.from_numpy(out_path[:, t - 1].astype(np.int64))]
        gates = torch.cat([x, h], dim=1) @ p['lstm_W'] + p['lstm_b']
        i, j, f, o = gates.split(D, dim=1)
        c = torch.sigmoid(f + 1.0) * c + torch.sigmoid(i) * torch.tanh(j)
        h = torch.sigmoid(o) * torch.tanh(c)
        if t == 0:
            intra = torch.zeros_like(h)
        elif t == 1:
            intra = outs[0]
        else:
            bef = torch.stack(outs, dim=1)
            sc = (p['intra_v'] * torch.tanh(bef @ p['intra_Wbef'] + (h @ p['intra_Wb'])[:, None, :] + p['intra_bias'])).sum(-1)
            intra = (torch.softmax(sc, dim=1)[:, :, None] * bef).sum(1)
        outs.append(h)
        pg = torch.softmax(_attention(p, 'glimpse', ref_g, h, intra), dim=1)
        q = (pg[:, :, None] * enc).sum(1)
        sc = _attention(p, 'pointer', ref_p, q, intra)
        any_special = (picked & special[None, :]).any(axis=1)
        allowed = loc[t // 3][None, :] & ~picked & ~(any_special[:, None] & special[None, :])
        lg = torch.where(torch.from_numpy(allowed), sc, torch.full_like(sc, PAD))
        logits.append(lg)
        out_path[:, t] = path[:, t] if path is not None else chooser(t, lg.detach().numpy().astype(np.float64))
        picked[np.arange(N), out_path[:, t]] = True
    return torch.stack(logits, dim=1), out_path


def decode_teacher(p, enc, path, dm, loc, special):
    """Teacher-forced logits [N, 9, A] along path."""
    return run_decoder(p, enc, dm, loc, special, path=np.asarray(path))[0]


def _params(flat, dm, dtype, grad=False):
    f = torch.tensor(np.asarray(flat), dtype=dtype, requires_grad=grad)
    return f, dm.split(f)


def logits_of(flat, obs, path, dm, loc, special, seed=0, step=0, pas=0, dtype=torch.float64):
    with torch.no_grad():
        _, p = _params(flat, dm, dtype)
        enc = encode(p, torch.tensor(np.asarray(obs), dtype=dtype), dm, seed, step, pas)
        return decode_teacher(p, enc, path, dm, loc, special).numpy()


def loss_and_grad(flat, obs, path, w, dm, loc, special, seed=0, step=0, pas=0, dtype=torch.float64):
    """-> dict(loss, grad [n_params], logits [N, 9, A]): mean_n(w_n * sum_t CE(logits[n, t], path[n, t]))"""
    f, p = _params(flat, dm, dtype, grad=True)
    enc = encode(p, torch.tensor(np.asarray(obs), dtype=dtype), dm, seed, step, pas)
    logits = decode_teacher(p, enc, path, dm, loc, special)
    tgt = torch.from_numpy(np.asarray(path, dtype=np.int64))
    ce = torch.logsumexp(logits, dim=2) - logits.gather(2, tgt[:, :, None])[:, :, 0]
    loss = (torch.tensor(np.asarray(w), dtype=dtype) * ce.sum(1)).mean()
    loss.backward()
    row_abs_mean = float((torch.tensor(np.asarray(w), dtype=dtype) * ce.sum(1)).abs().mean().detach())
    return dict(loss=float(loss.detach()), grad=f.grad.numpy().astype(np.float64), logits=logits.detach().numpy().astype(np.float64),
                row_abs_mean=row_abs_mean)


def loss_only(flat, obs, path, w, dm, loc, special):
    with torch.no_grad():
        lg = torch.from_numpy(logits_of(flat, obs, path, dm, loc, special))
        tgt = torch.from_numpy(np.asarray(path, dtype=np.int64))
        ce = torch.logsumexp(lg, dim=2) - lg.gather(2, tgt[:, :, None])[:, :, 0]
        return float((torch.tensor(np.asarray(w), dtype=torch.float64) * ce.sum(1)).mean())


# ---- picks ---------------------------------------------------------------------------------------------------------------
def top_two_gap(logits):
    """[N, 9] gap between the two largest logits of every row-step (allowed sets hold at least two items)."""
    s = np.sort(logits, axis=2)
    return s[:, :, -1] - s[:, :, -2]


def draw(logits, u):
    """Inverse CDF of softmax(logits) [N, 9, A] at u [N, 9]: the smallest allowed a whose inclusive prefix sum of exp(l - max)
    exceeds u * total -> (pick [N, 9], distance of u to the nearest CDF edge in units of the total)."""
    e = np.where(logits == PAD, 0.0, np.exp(logits - logits.max(axis=2, keepdims=True)))
    cdf = np.cumsum(e, axis=2)
    total = cdf[:, :, -1:]
    mass = u[:, :, None] * total
    last = (np.where(logits != PAD, np.arange(logits.shape[2]), -1)).max(axis=2)
    pick = np.minimum((cdf <= mass).sum(axis=2), last)
    edges = np.concatenate([np.zeros_like(total), cdf], axis=2) / total
    dist = np.abs(edges - u[:, :, None]).min(axis=2)
    return pick.astype(np.int32), dist


def sample_u(N, seed, step):
    """u [N, 9] of rl4rs_exactk_decode: uniform01(seed, step, row, t)"""
    return td3_ref.uniform01(seed, step, np.arange(N, dtype=np.uint64)[:, None], np.arange(T, dtype=np.uint64)[None, :])


def edge_bar(logit_bar):
    """As rainbow_ref.softq_edge_bar at temperature 1: logit errors up to eps move a normalised prefix by at most
    c (1 - c) (exp(2 eps) - 1) <= 0.55 eps for eps < 0.1; 1e-5 covers the fp32 rounding of the prefix sum of up to 512 terms."""
    assert logit_bar < 0.1
    return 0.55 * logit_bar + 1e-5


def decode(flat, obs, dm, loc, special, greedy, seed=0, step=0, pas=1, dtype=torch.float64):
    """The restatement's own slates -> path [N, 9] (first maximum, or the inverse-CDF draw at sample_u)."""
    u = sample_u(len(obs), seed, step)
    chooser = (lambda t, lg: lg.argmax(axis=1)) if greedy else (lambda t, lg: draw(lg[:, None, :], u[:, t:t + 1])[0][:, 0])
    with torch.no_grad():
        _, p = _params(flat, dm, dtype)
        enc = encode(p, torch.tensor(np.asarray(obs), dtype=dtype), dm, seed, step, pas)
        return run_decoder(p, enc, dm, loc, special, chooser=chooser)[1]


# ---- critic and Adam -----------------------------------------------------------------------------------------------------
def critic_loss_and_grad(flat, obs, target, od=256, hidden=128, dtype=torch.float64):
    """-> (value [N], err [N] = (value - target)^2, gradient of sum(err))"""
    f = torch.tensor(np.asarray(flat), dtype=dtype, requires_grad=True)
    p = NX.critic_split(f, od, hidden)
    h = torch.tensor(np.asarray(obs), dtype=dtype)
    for i in (1, 2, 3):
        h = torch.relu(h @ p['W%d' % i] + p['b%d' % i])
    v = (h @ p['W4'] + p['b4'])[:, 0]
    err = (v - torch.tensor(np.asarray(target), dtype=dtype)) ** 2
    err.sum().backward()
    return v.detach().numpy().astype(np.float64), err.detach().numpy().astype(np.float64), f.grad.numpy().astype(np.float64)


# seeds of the critic comparisons' inputs per row count: 70 + N, but for N = 4099.  Seed 4169 puts one unit of the second layer at
# 1.5e-7 from 0 (0.42 rms of the float32 pre-activation error) with 1.05e-4 of the gradient's max-norm behind it; the float32
# restatement lands on either side of it from one CPU to the next, its gradient error is 1.1e-7 or 3.9e-4, and the bar moves with it.
# 4175 is the first seed from there that keeps every unit carrying at least 2^-23 of the max-norm (a flip would show above the
# rounding level) CRITIC_KINK_MARGIN = BAR_FACTOR rms off 0: four standard deviations of a float32 pre-activation error, which the
# 1.6 M units of this size still allow.  tests/test_exactk_host.py holds every row count to it.
CRITIC_SEEDS = {37: 107, 1: 71, 300: 370, 4099: 4175}
CRITIC_KINK_MARGIN = BAR_FACTOR


def critic_case(N, od=256, hidden=128):
    """(flat parameters, obs [N, od], target [N]) of the critic comparisons, float32"""
    rs = np.random.RandomState(CRITIC_SEEDS[N])
    flat = NX.init_critic_params(od, hidden, 5) + (0.05 * rs.randn(NX.critic_param_count(od, hidden))).astype(np.float32)
    return flat, rs.randn(N, od).astype(np.float32), (3.0 * rs.randn(N)).astype(np.float32)


def critic_relu_sites(flat, obs, target, od=256, hidden=128):
    """relu_sites for the critic's three hidden layers (critic_loss_and_grad, restated with its pre-activations kept)"""
    def run(dtype):
        f = torch.tensor(np.asarray(flat), dtype=dtype, requires_grad=True)
        p = NX.critic_split(f, od, hidden)
        h, kept = torch.tensor(np.asarray(obs), dtype=dtype), []
        for i in (1, 2, 3):
            z = h @ p['W%d' % i] + p['b%d' % i]
            h = torch.relu(z)
            h.retain_grad()
            kept.append((z.detach().numpy().reshape(-1).astype(np.float64), h))
        v = (h @ p['W4'] + p['b4'])[:, 0]
        ((v - torch.tensor(np.asarray(target), dtype=dtype)) ** 2).sum().backward()
        return kept, np.abs(f.grad.numpy().astype(np.float64)).max()
    (k64, gmax), (k32, _) = run(torch.float64), run(torch.float32)
    return [dict(name='layer%d' % (i + 1), z=np.abs(z), g=np.abs(h.grad.numpy().reshape(-1)) / gmax,
                 rms=float(np.sqrt(np.mean((z32 - z) ** 2)))) for i, ((z, h), (z32, _)) in enumerate(zip(k64, k32))]


def adam_tf(p, g, m, v, t, lr, b1=0.9, b2=0.98, eps=1e-8):
    """tf.train.AdamOptimizer step t (1-based) -> (p, m, v)"""
    lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


# ---- host logic of the trainer, restated ---------------------------------------------------------------------------------
def best_of(rewards):
    """index [N] of the kept climb: the larger reward, ties to the first (sorted(..., reverse=True)[0] is stable)."""
    return np.argmax(np.asarray(rewards), axis=0)


def advantage(reward, baseline):
    """-> (advantage / population std, skip): skip when the std is 0 or not finite."""
    adv = np.asarray(reward, dtype=np.float64) - np.asarray(baseline, dtype=np.float64)
    sd = adv.std()
    if not np.isfinite(sd) or sd == 0:
        return adv, True
    return adv / sd, False


# ---- cases ---------------------------------------------------------------------------------------------------------------
# (A, H, heads, blocks, N).  Shapes 0 - 3 stay in the single-chunk form of every sample-axis reduction; shapes 4 - 6 are each the
# smallest that crosses the thresholds sample_axis_forms() names (tests/test_exactk_host.py asserts the form of each):
#   4  (75, 32, 2, 1, 900)    everything but the decoder's 9 N threshold
#   5  (40, 16, 2, 1, 1900)   the decoder's 9 N threshold as well, M = 76 000
#   6  (284, 64, 4, 2, 66)    the reference's own widths past M > 16384 and N > 64; dropout 0.1 only, as the trainer runs it
GPU_SHAPES = ((284, 64, 4, 2, 37), (75, 32, 2, 1, 5), (284, 64, 4, 2, 1), (64, 16, 2, 2, 33), (75, 32, 2, 1, 900), (40, 16, 2, 1, 1900),
              (284, 64, 4, 2, 66))
RATES = (0.0, 0.1)


def sample_axis_forms(A, N):
    """The chunk rules of csrc/exactk.hip's sample-axis reductions, restated as arithmetic on (A, N) with M = N A rows of items:
    xk_colsum splits Ns rows into chunks of max(64, ceil(Ns / XK_COLSUM_CHUNKS = 1024)) rows, xk_tn and the critic into chunks of
    max(256, ceil(Ns / 64) rounded up to 16); more than one chunk means partials joined by k_reduce_chunks.  k_xk_loss walks the N
    rows with a stride of 256.  Whoever retunes one of these rules rechooses GPU_SHAPES 4 - 6 with this function."""
    ceil = lambda a, b: (a + b - 1) // b
    colsum = lambda ns: max(64, ceil(ns, 1024))
    tn = lambda ns: max(256, ceil(ceil(ns, 64), 16) * 16)
    M = N * A
    return dict(colsum_rows_chunks=ceil(N, colsum(N)),                 # init_c, init_h, first input: > 1 from N > 64
                tn_rows_chunks=ceil(N, tn(N)),                         # user layer, the critic's four gradients: > 1 from N > 256
                loss_trips=ceil(N, 256),                               # k_xk_loss: > 1 from N > 256
                tn_items_chunk=tn(M),                                  # > 256 from M > 16384
                colsum_items_chunk=colsum(M),                          # > 64 from M > 65536; no multiple of 8: a partial last trip
                tn_decoder_chunk=tn(T * N))                            # > 256 from 9 N > 16384


# seeds per (shape, dropout rate), chosen by two conditions on the restatement alone (three for shapes 4 - 6, below).  (1) The fp32 yardstick is not dominated by one
# tensor, i.e. by a relu unit of the 13 M of the largest shape that float32 puts on the other side of 0: the yardstick is meant to
# be the rounding level.  (2) That holds by more than one accumulation order's luck: rounding_variants() repeats the float32 run
# with every parameter moved by one float32 rounding, which moves the pre-activations about as much as another accumulation order
# does, and the gradient error has to stay inside the bar in all of them (on (0, 0.1) seed 20 meets (1) and misses (2) at its
# fourth variant, 1.2e-5; seed 29 meets both).  tests/test_exactk_host.py checks both conditions for every case.
# Shapes 4 - 6 have 2.4 M to 8.6 M relu units in a layer, and (1) and (2) no longer keep a case off a relu kink there: about
# 5e6 d of the units that carry the gradient bar lie within d of 0, so every seed has a few within the float32 error of a
# pre-activation (rms 2e-7 to 4e-7), and five float32 runs that leave such a unit's sign alone say little about a sixth order of
# accumulation.  On (5, 0.1) seed 144 meets (1) and (2) with one V unit of block 0 at 7.4e-8 (0.32 rms) and 4.09e-5 of the gradient's
# max-norm behind it; the device puts it on the other side of 0, and its gradient then differs by 5.2e-5 in exactly d Wv, d bv (by
# 4.09e-5), d table and the user layer, every other tensor at the rounding level.  Hence (3), for these shapes (KINK_KEYS): every
# unit that carries at least the gradient bar lies farther from 0 in float64 than KINK_MARGIN = 1 rms of the float32 restatement's
# pre-activation error at its layer (relu_sites; tests/test_exactk_host.py).  One rms is what a search can still meet at these unit
# counts (one seed in five of those that meet (1)); it leaves about one chance in six per such unit that another
# float32 order flips it.  A flip shows as above: an error confined to the tensors at and below one relu layer that equals one
# unit's g, which relu_sites lists.  Shapes 0 - 3 were chosen before (3) and are not held to it ((0, 0.1) sits at 0.28 rms).
# Seeds searched upward from 31 (shape 4), 60 (shape 5) and 70 (shape 6); 34 meets (1) and (2) on (4, 0.0) and misses (3) at 0.39 rms.
# (5, 0.1) also has to leave room for a decode stream (DECODE_STREAMS): on the seeds that meet (1) and (2) between 20 and 50 of the
# 1900 greedy rows have a top-two gap under 10 logit bars, the cap being 19; 170 is the first seed from 145 that meets all of it.
ROUNDING_VARIANTS = 4
KINK_MARGIN = 1.0
CASE_SEEDS = {(0, 0.0): 22, (0, 0.1): 29, (1, 0.0): 30, (1, 0.1): 30, (2, 0.0): 40, (2, 0.1): 40, (3, 0.0): 50, (3, 0.1): 50,
              (4, 0.0): 37, (4, 0.1): 38, (5, 0.0): 66, (5, 0.1): 170, (6, 0.1): 97}
CASE_KEYS = tuple(sorted(CASE_SEEDS))          # every (shape index, rate) that is a case: the tests' parametrisation
DECODE_SHAPES = tuple(i for i in range(len(GPU_SHAPES)) if (i, 0.1) in CASE_SEEDS)
KINK_KEYS = tuple(k for k in CASE_KEYS if k[0] >= 4)
CRAFTED = (3, 50)                  # (shape index, seed) of the zero-row case, dropout 0
TINY_SHAPE = (11, 16, 2, 1, 3)
# (seed, step) of the decode comparisons per shape: streams on which the restatement's own slates keep the exclusion caps
# (tests/test_exactk_host.py); (3, 11) leaves one of the 37 rows of shape 0 with a greedy near-tie.  Shape 4: (3, 11) to (3, 13) leave
# 10, 11 and 14 of the 900 rows with one, (3, 14) leaves 9; shape 5: (3, 12) leaves 18 of the 1900
DECODE_STREAMS = ((3, 12), (3, 11), (3, 11), (3, 11), (3, 14), (3, 12), (3, 11))


def case(i, rate):
    return make_case(GPU_SHAPES[i], CASE_SEEDS[(i, rate)], rate)


def crafted_case():
    return make_case(GPU_SHAPES[CRAFTED[0]], CRAFTED[1], 0.0, crafted=True)


def synth_masks(A):
    """location_mask [3, A] and is_special [A] of the synthetic catalogue (A = 284)"""
    import os
    from rl4rs_amd.data import CatalogTables
    cat = CatalogTables(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'catalog_synth.csv'), A)
    return np.asarray(cat.location_mask[:3]).astype(bool), np.asarray(cat.is_special).astype(bool)


def random_masks(A, rs, usable=12):
    if A >= 36:
        special = rs.rand(A) < 0.15
    else:
        special = np.zeros(A, dtype=bool)
        special[rs.randint(A)] = True
    loc = rs.rand(3, A) < 0.45
    for l in range(3):
        free = np.nonzero(~special)[0]
        loc[l, rs.choice(free, size=min(usable, len(free)), replace=False)] = True
    return loc, special


def make_case(shape, seed, rate=0.0, crafted=False):
    A, H, heads, blocks, N = shape
    rs = np.random.RandomState(seed)
    dm = Dims(A, H, heads, blocks, rate=rate)
    loc, special = synth_masks(A) if A == 284 else random_masks(A, rs, usable=12 if A >= 36 else 9)
    flat = NX.init_exactk_params(dm.od, H, blocks, dm.vocab, seed).astype(np.float64)
    p = dm.split(flat)
    for name, _, init in NX.shapes(dm.od, H, blocks, dm.vocab):       # biases, states and layer norm off their trivial values
        if init in ('zeros', 'ones'):
            p[name] += 0.1 * rs.randn(*p[name].shape)
    obs = rs.randn(N, dm.od)
    if crafted:
        # the user half all zero (a bias far below every pre-activation) and one zero table row: that candidate's key / query row of
        # block 0 sums to exactly 0
        p['user_b'][:] = -1e3
        p['table'][3] = 0.0
    flat = flat.astype(np.float32)
    obs = obs.astype(np.float32)
    path = random_slates(N, loc, special, rs)
    w = rs.randn(N).astype(np.float32)
    return dict(dm=dm, loc=loc, special=special, flat=flat, obs=obs, path=path, w=w, N=N, shape=shape)


def fp32_yardstick(c, seed=0, step=0, pas=0):
    """Errors of the float32 restatement against the float64 one on the inputs of case c:
    logit (max abs over the allowed entries), loss (abs; the largest of this run and the rounding_variants runs, since one float32
    sum can land on the float64 value by luck), grad_rel (max abs over the whole gradient / its max-norm), and the
    largest single tensor's share, to spot a case dominated by one relu kink flip."""
    a = loss_and_grad(c['flat'], c['obs'], c['path'], c['w'], c['dm'], c['loc'], c['special'], seed, step, pas, torch.float64)
    b = loss_and_grad(c['flat'], c['obs'], c['path'], c['w'], c['dm'], c['loc'], c['special'], seed, step, pas, torch.float32)
    ok = a['logits'] != PAD
    gmax = np.abs(a['grad']).max()
    per = dict((n, float(np.abs(x - y).max() / gmax)) for (n, x), y in
               zip(c['dm'].split(a['grad']).items(), c['dm'].split(b['grad']).values()))
    loss_err = max([abs(a['loss'] - b['loss'])] + rounding_variants(c, a, seed, step, pas)[1])
    return dict(logit=float(np.abs(a['logits'] - b['logits'])[ok].max()), loss=loss_err,
                grad_rel=float(np.abs(a['grad'] - b['grad']).max() / gmax), per_tensor=per, ref=a)


def rounding_variants(c, ref, seed=0, step=0, pas=0):
    """ROUNDING_VARIANTS float32 runs whose parameters are flat * (1 + 2^-24 g), g standard normal (fixed streams), against the
    float64 reference ``ref`` of the unperturbed case -> (gradient errors relative to the float64 gradient's max-norm, loss errors)"""
    gmax = np.abs(ref['grad']).max()
    g_err, l_err = [], []
    for k in range(ROUNDING_VARIANTS):
        g = np.random.RandomState(100 + k).randn(len(c['flat']))
        flat = (c['flat'].astype(np.float64) * (1.0 + 2.0 ** -24 * g)).astype(np.float32)
        b = loss_and_grad(flat, c['obs'], c['path'], c['w'], c['dm'], c['loc'], c['special'], seed, step, pas, torch.float32)
        g_err.append(float(np.abs(ref['grad'] - b['grad']).max() / gmax))
        l_err.append(abs(ref['loss'] - b['loss']))
    return g_err, l_err


def relu_sites(c, seed=0, step=0, pas=0):
    """Every relu of the encoder (the user layer, then Q, K, V and the feed-forward layer of each block), for the third condition on
    a case's seed -> list of dict(name, z = |float64 pre-activation| per unit, g = |d loss / d output| per unit over the gradient's
    max-norm, rms = root mean square of the float32 restatement's pre-activation error at the site).  A unit whose float32 sign
    differs from its float64 sign moves its layer's bias gradient by g of the max-norm, and the weight and input gradients with it."""
    global RELU_TAP
    args = (c['flat'], c['obs'], c['path'])
    seen = {torch.float64: [], torch.float32: []}
    try:
        RELU_TAP = lambda z, o: (o.retain_grad(), seen[torch.float64].append((z, o)))
        ref = loss_and_grad(*args, c['w'], c['dm'], c['loc'], c['special'], seed, step, pas, torch.float64)
        RELU_TAP = lambda z, o: seen[torch.float32].append(z)
        logits_of(*args, c['dm'], c['loc'], c['special'], seed, step, pas, torch.float32)
    finally:
        RELU_TAP = None
    gmax = np.abs(ref['grad']).max()
    names = ['user'] + ['blk%d_%s' % (b, n) for b in range(c['dm'].blocks) for n in ('Q', 'K', 'V', 'ffn')]
    assert len(names) == len(seen[torch.float64]) == len(seen[torch.float32])
    out = []
    for name, (z, o), z32 in zip(names, seen[torch.float64], seen[torch.float32]):
        z = z.detach().numpy().reshape(-1)
        out.append(dict(name=name, z=np.abs(z), g=np.abs(o.grad.numpy().reshape(-1)) / gmax,
                        rms=float(np.sqrt(np.mean((z32.numpy().reshape(-1).astype(np.float64) - z) ** 2)))))
    return out


# fp32_yardstick(case, seed=5, step=7) - the dropout stream the GPU tests use - per (shape index, rate) and of the crafted case,
# measured on the CPU
# (tests/test_exactk_host.py reproduces them within a factor of 2)
MEASURED = {
    (0, 0.0): dict(logit=1.28e-06, loss=5.3e-07, grad_rel=1.13e-06),
    (0, 0.1): dict(logit=1.85e-06, loss=1.1e-06, grad_rel=1.1e-06),
    (1, 0.0): dict(logit=8.67e-07, loss=1.21e-06, grad_rel=6.3e-07),
    (1, 0.1): dict(logit=8.84e-07, loss=2.42e-06, grad_rel=5.31e-07),
    (2, 0.0): dict(logit=7.93e-07, loss=1.03e-06, grad_rel=1.65e-06),
    (2, 0.1): dict(logit=8.73e-07, loss=5.05e-07, grad_rel=1.07e-06),
    (3, 0.0): dict(logit=1.48e-06, loss=4.14e-07, grad_rel=7.93e-07),
    (3, 0.1): dict(logit=1.37e-06, loss=3.91e-07, grad_rel=9.89e-07),
    (4, 0.0): dict(logit=1.66e-06, loss=1.75e-07, grad_rel=1.37e-06),
    (4, 0.1): dict(logit=1.86e-06, loss=2.72e-07, grad_rel=8.14e-07),
    (5, 0.0): dict(logit=1.79e-06, loss=1.98e-07, grad_rel=8.05e-07),
    (5, 0.1): dict(logit=1.18e-06, loss=1.06e-07, grad_rel=7.57e-07),
    (6, 0.1): dict(logit=1.45e-06, loss=1.15e-06, grad_rel=1.06e-06),
    'crafted': dict(logit=6.23e-07, loss=1.2e-06, grad_rel=5.52e-07),
}


def bars(key, ref=None):
    """(logit bar, loss bar, gradient bar relative to the reference gradient's max-norm) of a case: BAR_FACTOR x the measured fp32
    error, nothing else."""
    m = MEASURED[key]
    return BAR_FACTOR * m['logit'], BAR_FACTOR * m['loss'], BAR_FACTOR * m['grad_rel']


# ---- "it learns": REINFORCE with the critic baseline on a reward computed from the path ----------------------------------------
LEARN_SHAPE = (75, 32, 2, 1, 64)
LEARN_SEED = 60
LEARN_UPDATES = 30
LEARN_REF_GAIN = 4.203125          # 4.796875 -> 9.0, measured with RefBackend (float32, CPU)


def learn_setup():
    c = make_case(LEARN_SHAPE, LEARN_SEED, 0.0)
    rs = np.random.RandomState(LEARN_SEED + 1)
    free = np.nonzero(~c['special'])[0]
    favoured = np.zeros(c['dm'].A, dtype=bool)
    favoured[rs.choice(free, size=len(free) // 2, replace=False)] = True
    c['flat'] = NX.init_exactk_params(c['dm'].od, c['dm'].H, c['dm'].blocks, c['dm'].vocab, LEARN_SEED)
    c['critic'] = NX.init_critic_params(c['dm'].od, 128, LEARN_SEED + 2)
    c['favoured'] = favoured
    return c


def learn_loop(backend, favoured, updates):
    """backend: sample(step) -> path, greedy() -> path, critic_update(reward) -> baseline before the update, gen_update(path, w, step).
    -> (mean greedy reward before, after)"""
    score = lambda path: favoured[np.asarray(path)].sum(axis=1).astype(np.float64)
    before = score(backend.greedy()).mean()
    for k in range(updates):
        path = backend.sample(k)
        reward = score(path)
        baseline = backend.critic_update(reward)
        w, skip = advantage(reward, baseline)
        if not skip:
            backend.gen_update(path, w, k)
    return before, score(backend.greedy()).mean()


class RefBackend(object):
    """The float32 CPU restatement behind learn_loop."""

    def __init__(self, c, dtype=torch.float32):
        self.c, self.dtype = c, dtype
        self.flat = c['flat'].astype(np.float64)
        self.cflat = c['critic'].astype(np.float64)
        self.gm, self.gv, self.gt = np.zeros_like(self.flat), np.zeros_like(self.flat), 0
        self.cm, self.cv, self.ct = np.zeros_like(self.cflat), np.zeros_like(self.cflat), 0

    def sample(self, step):
        c = self.c
        return decode(self.flat, c['obs'], c['dm'], c['loc'], c['special'], False, seed=0, step=step, dtype=self.dtype)

    def greedy(self):
        c = self.c
        return decode(self.flat, c['obs'], c['dm'], c['loc'], c['special'], True, dtype=self.dtype)

    def critic_update(self, reward):
        v, _, g = critic_loss_and_grad(self.cflat, self.c['obs'], reward, dtype=self.dtype)
        self.ct += 1
        self.cflat, self.cm, self.cv = adam_tf(self.cflat, g, self.cm, self.cv, self.ct, 5e-3)
        return v

    def gen_update(self, path, w, step):
        c = self.c
        g = loss_and_grad(self.flat, c['obs'], path, w, c['dm'], c['loc'], c['special'], dtype=self.dtype)['grad']
        self.gt += 1
        self.flat, self.gm, self.gv = adam_tf(self.flat, g, self.gm, self.gv, self.gt, 1e-3)
