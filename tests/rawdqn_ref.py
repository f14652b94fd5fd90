"""float64 restatement of the on-device raw-state DQN (include/rl4rs_hip.h, "On-device raw-state DQN"): the packed record layout,
the raw-state model (rl4rs/nets/rllib/rllib_rawstate_model.py:25-86 under the mask wrapper rllib_mask_model.py:67-115), the
(double-)Q Huber loss of tests/dqn_ref.py on it with torch autograd for the gradient, and the per-variable-clipped Adam step.

Test infrastructure only.  PARITY UNPINNED like tests/dqn_ref.py (ray 1.5.1 is absent).  ``dtype=np.float32`` runs the same code in
single precision: the tests measure that run against the float64 one and allow the device a multiple of it.

Ids are clamped to [0, H) where the tables are read, as every device forward does; the record keeps them as they come."""
import numpy as np

F32_MIN = float(np.finfo(np.float32).min)
ORDER = ('cat_emb', 'seq_emb', 'dense_w1', 'dense_b1', 'dense_w2', 'dense_b2', 'ctx_w', 'ctx_b', 'head_w', 'head_b')
TABLES = ('cat_emb', 'seq_emb')


# ---- record ----------------------------------------------------------------------------------------------------------
def record_fields(cfg):
    """-> (REC, {field: (offset, words)}) of [dense Dn | cat Cn | seq_0 L | ... | seq_{S-1} L | zero pad to a multiple of 4]."""
    Dn, Cn, L, S = cfg['dense_feature_num'], cfg['category_feature_num'], cfg['maxlen'], cfg['seq_num']
    fields = {'dense': (0, Dn), 'cat': (Dn, Cn)}
    for s in range(S):
        fields['seq%d' % s] = (Dn + Cn + s * L, L)
    used = Dn + Cn + S * L
    rec = (used + 3) // 4 * 4
    fields['pad'] = (used, rec - used)
    return rec, fields


def pack_records(cfg, cat, dense, seqs):
    """-> int32 [N, REC]: the record's 32-bit words (the dense part holds the float32 bit patterns)."""
    rec, f = record_fields(cfg)
    N = len(cat)
    out = np.zeros((N, rec), dtype=np.int32)
    o, n = f['dense']
    out[:, o:o + n] = np.ascontiguousarray(dense, dtype=np.float32).view(np.int32)
    o, n = f['cat']
    out[:, o:o + n] = np.asarray(cat, dtype=np.int32)
    for s, q in enumerate(seqs):
        o, n = f['seq%d' % s]
        out[:, o:o + n] = np.asarray(q, dtype=np.int32)
    return out


def unpack_records(cfg, rec):
    """int32 [N, REC] -> (cat int32 [N, Cn], dense float32 [N, Dn], [seq int32 [N, L]] * S)"""
    _, f = record_fields(cfg)
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    o, n = f['dense']
    dense = np.ascontiguousarray(rec[:, o:o + n]).view(np.float32)
    o, n = f['cat']
    cat = rec[:, o:o + n].copy()
    seqs = []
    for s in range(cfg['seq_num']):
        o, n = f['seq%d' % s]
        seqs.append(rec[:, o:o + n].copy())
    return cat, dense, seqs


def as_words(rec_f32):
    """float32 [N, REC] as it leaves the device -> its int32 words"""
    return np.ascontiguousarray(rec_f32).view(np.int32)


# ---- model -----------------------------------------------------------------------------------------------------------
def flat_weights(w):
    """init_rawpolicy_weights' dict -> the handle's ten variables (head_w = [out_w | value_w], head_b = [out_b | value_b])"""
    out = dict((k, np.asarray(w[k])) for k in ORDER[:8])
    out['head_w'] = np.concatenate([w['out_w'], w['value_w']], axis=1)
    out['head_b'] = np.concatenate([w['out_b'], w['value_b']])
    return out


def split_flat(flat, cfg):
    """the handle's flat buffer -> its ten variables"""
    H, E, U = cfg['category_hash_size'], cfg['emb_size'], cfg['hidden_units']
    Dn, S, A = cfg['dense_feature_num'], cfg['seq_num'], cfg['action_size']
    shapes = [(H, E), (H, E), (Dn, U), (U,), (U, U), (U,), (S * E + U + E, 256), (256,), (256, A + 1), (A + 1,)]
    out, o = {}, 0
    for name, shp in zip(ORDER, shapes):
        k = int(np.prod(shp))
        out[name] = np.asarray(flat[o:o + k]).reshape(shp)
        o += k
    assert o == len(flat)
    return out


def unpack_bits(bits, A):
    b = np.ascontiguousarray(bits).view(np.uint32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :A].astype(np.float64)


def _tdt(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def q_values(v, cfg, cat, dense, seqs, dtype=np.float64):
    """Unmasked Q rows [N, A] (torch, differentiable in the torch tensors of ``v``) of the ten variables ``v``."""
    import torch
    tdt = _tdt(dtype)
    H, A = cfg['category_hash_size'], cfg['action_size']
    ids = lambda x: torch.as_tensor(np.clip(np.asarray(x, dtype=np.int64), 0, H - 1))
    elu = torch.nn.functional.elu
    seq_feat = [v['seq_emb'][ids(s)].mean(dim=1) for s in seqs]
    x = torch.as_tensor(np.asarray(dense, dtype=np.float32)).to(tdt)
    d = elu(elu(x @ v['dense_w1'] + v['dense_b1']) @ v['dense_w2'] + v['dense_b2'])
    c = v['cat_emb'][ids(cat)].mean(dim=1)
    ctx = elu(torch.cat(seq_feat + [d, c], dim=1) @ v['ctx_w'] + v['ctx_b'])
    return (ctx @ v['head_w'] + v['head_b'])[:, :A]


def masked(q, mask, dtype=np.float64):
    """q + max(log(mask), float32.min) in ``dtype`` (numpy)"""
    q = np.asarray(q, dtype=dtype)
    if mask is None:
        return q
    with np.errstate(divide='ignore'):
        return q + np.maximum(np.log(np.asarray(mask, dtype=dtype)), np.dtype(dtype).type(F32_MIN))


def greedy(v, cfg, cat, dense, seqs, mask, dtype=np.float64):
    """-> (first maximum of the masked Q row, the masked rows)"""
    import torch
    tdt = _tdt(dtype)
    tv = dict((k, torch.as_tensor(np.asarray(x)).to(tdt)) for k, x in v.items())
    with torch.no_grad():
        q = masked(q_values(tv, cfg, cat, dense, seqs, dtype).numpy(), mask, dtype)
    return q.argmax(axis=1), q


def loss_and_grad(v, tv, cfg, rec, act, rew, done, next_rec, next_mask, weights=None, gamma=1.0, double_q=True, dtype=np.float64,
                  want_grad=True, astar=None):
    """-> dict(loss, grad {variable: array}, td, y, qsa, astar (-1 on terminal rows), boot, gap, q_sel, stats).
    astar: the a* to bootstrap from on the rows that do, instead of the first maximum found here (a caller that has settled a
    near-tie some other way); ``gap`` and ``q_sel`` still describe the maxima found here.
    v / tv: the ten variables of the online / target net; rec / next_rec int32 [N, REC]; next_mask [N, A] of 0 / 1 or None.
    A terminal row's successor record is not read (zeros stand in for it); a non-terminal row whose successor allows no action gets
    y = r.  q_sel: the masked Q(s') rows of the selecting net, gap: their top-two gap on the rows that bootstrap (inf elsewhere)."""
    import torch
    tdt = _tdt(dtype)
    t = lambda x: torch.as_tensor(np.asarray(x)).to(tdt)
    N = len(act)
    A = cfg['action_size']
    done_b = np.asarray(done).astype(bool)
    on = dict((k, t(x).clone().requires_grad_(want_grad)) for k, x in v.items())
    tg = dict((k, t(x)) for k, x in tv.items())
    nrec = np.where(done_b[:, None], 0, np.asarray(next_rec, dtype=np.int32)).astype(np.int32)
    mask = np.ones((N, A)) if next_mask is None else np.asarray(next_mask, dtype=np.float64)
    with torch.no_grad():
        nxt = unpack_records(cfg, nrec)
        q_t = q_values(tg, cfg, *nxt, dtype=dtype).numpy()
        q_o = q_values(dict((k, x.detach()) for k, x in on.items()), cfg, *nxt, dtype=dtype).numpy() if double_q else q_t
    q_sel = masked(q_o, mask, dtype)
    boot = ~done_b & (mask > 0).any(axis=1)
    a_ref = q_sel.argmax(axis=1)
    if astar is not None:
        a_ref = np.where(boot, np.asarray(astar, dtype=np.int64), a_ref)
    top = np.sort(q_sel.astype(np.float64), axis=1)[:, -2:]
    gap = np.where(boot, top[:, 1] - top[:, 0], np.inf)
    qt = np.where(boot, q_t[np.arange(N), a_ref], 0).astype(dtype)
    r = np.asarray(rew, dtype=np.float32).astype(dtype)
    y = np.where(boot, r + np.dtype(dtype).type(gamma) * qt, r).astype(dtype)
    q_s = q_values(on, cfg, *unpack_records(cfg, rec), dtype=dtype)
    qsa = q_s.gather(1, torch.as_tensor(np.asarray(act, dtype=np.int64))[:, None])[:, 0]
    td = qsa - t(y)
    ad = td.abs()
    hub = torch.where(ad < 1.0, 0.5 * td * td, ad - 0.5)
    w = torch.ones(N, dtype=tdt) if weights is None else t(np.asarray(weights, dtype=np.float32))
    loss = (w * hub).mean()
    grad = None
    if want_grad:
        loss.backward()
        grad = dict((k, on[k].grad.numpy()) for k in ORDER)
    stats = np.array([(w * hub).sum().item(), qsa.sum().item(), float(y.astype(np.float64).sum()), ad.sum().item()])
    return dict(loss=loss.item(), grad=grad, td=td.detach().numpy(), y=y, qsa=qsa.detach().numpy(), astar=np.where(done_b, -1, a_ref),
                boot=boot, gap=gap, q_sel=q_sel, stats=stats)


# ---- optimiser -------------------------------------------------------------------------------------------------------
def var_norms(grad):
    """float64 norms of the ten variables of ``grad`` (a dict) in flat order"""
    return np.array([np.sqrt((np.asarray(grad[k], dtype=np.float64) ** 2).sum()) for k in ORDER])


def adam_clip_by_var_first_step(params, grad, lr, var_clip, beta1=0.9, beta2=0.999, eps=1e-8):
    """Closed form of the FIRST TF-form Adam step from zero moments with tf.clip_by_norm per variable -> dict of new parameters."""
    out = {}
    lr_t = lr * np.sqrt(1 - beta2) / (1 - beta1)
    for k in ORDER:
        g = np.asarray(grad[k], dtype=np.float64)
        norm = np.sqrt((g ** 2).sum())
        if var_clip > 0 and norm > var_clip:
            g = g * (var_clip / norm)
        out[k] = np.asarray(params[k], dtype=np.float64) - lr_t * ((1 - beta1) * g) / (np.sqrt((1 - beta2) * g * g) + eps)
    return out
