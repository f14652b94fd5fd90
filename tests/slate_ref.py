"""float64 restatement (torch autograd) of the slate-wise supervised models of script/supervised_train.py - test infrastructure.

The trunks are those of oracle/simnets.py / oracle/dien.py (``loss_and_grad`` there; copied, since those functions end in the
item-wise loss); the heads follow rl4rs/nets/*_slate.py, *_slate_multiclass.py and adversarial_slate.py:

* 'item'         Dense(class_num, softmax) + keras binary_crossentropy of the clipped probabilities (the existing trainers)
* 'slate'        Dense(9, sigmoid) + binary_crossentropy
* 'multiclass'   Dense(22, softmax) + categorical_crossentropy(one_hot(y . [1,2,4,1,2,4,1,2,4], 22), .)
* 'adversarial'  adversarial_slate.py: [mean of each sequence's embeddings | dense tower | mean of the category embeddings without
                 the last id] -> Dense(9, sigmoid); loss = 0.1 * binary_crossentropy + sum_j softmax(sigmoid)_j (1 - y_j)

PARITY UNPINNED, as the item-wise loss is: TensorFlow 1.15 cannot run here.  The two rules restated from
tensorflow/python/keras/backend.py (1.15) **[from memory]**: ``binary_crossentropy(target, output)`` - when ``output`` is the
result of a ``Sigmoid`` op (and not an EagerTensor / Variable) it takes that op's input as logits and returns
``sigmoid_cross_entropy_with_logits`` = max(x, 0) - x y + log(1 + exp(-|x|)), without clipping; ``categorical_crossentropy`` does the
same for a ``Softmax`` op with ``softmax_cross_entropy_with_logits_v2`` = logsumexp(x) - x[c].  Both models end in such an op
(``Dense(.., activation='sigmoid' / 'softmax')``), so the losses here are written from the logits.
"""
import numpy as np

CLASS_WEIGHTS = (1, 2, 4, 1, 2, 4, 1, 2, 4)


def slate_class(labels):
    return (np.asarray(labels) != 0).astype(np.int64) @ np.asarray(CLASS_WEIGHTS, dtype=np.int64)


def _trunk(torch, algo, w, cfg, dense, cat, seqs, mask1, mask2, rate):
    """-> the input of the output layer ('simulator_obs'; for the adversarial model its feature concat)"""
    elu = torch.nn.functional.elu
    sig = torch.sigmoid
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    i64 = lambda a: torch.tensor(np.asarray(a, dtype=np.int64))
    x, ids = f64(dense), i64(cat)
    N = ids.shape[0]
    h = elu(x @ w['dense_w1'] + w['dense_b1'])
    if mask1 is not None:
        h = h * f64(mask1) / (1.0 - rate)
    h = elu(h @ w['dense_w2'] + w['dense_b2'])
    if mask2 is not None:
        h = h * f64(mask2) / (1.0 - rate)
    if algo == 'dnn':
        feat = torch.cat([w['cat_emb'][ids].mean(dim=1), h], dim=1)
        a = elu(feat @ w['fc_w'] + w['fc_b'])
        return elu(a @ w['obs_w'] + w['obs_b'])
    if algo == 'widedeep':
        pooled = torch.cat([w['seq_emb'][i64(q)].mean(dim=1) for q in seqs], dim=1)
        return torch.cat([elu(pooled @ w['fc_w'] + w['fc_b']), h, w['cat_emb'][ids].reshape(N, -1)], dim=1)
    if algo == 'adversarial_slate':
        pooled = [w['seq_emb'][i64(q)].mean(dim=1) for q in seqs]
        return torch.cat(pooled + [h, w['cat_emb'][ids[:, :-1]].mean(dim=1)], dim=1)
    if algo == 'lstm':
        def gru_last(X, i):
            k, r, b = w[i + '_kernel'], w[i + '_recurrent'], w[i + '_bias']
            U = r.shape[0]
            hs = lambda v: torch.clamp(0.2 * v + 0.5, 0.0, 1.0)
            hst = torch.zeros((X.shape[0], U), dtype=torch.float64)
            for t in range(X.shape[1]):
                xp = X[:, t] @ k + b
                hz = hst @ r[:, :2 * U]
                z = hs(xp[:, :U] + hz[:, :U])
                rr = hs(xp[:, U:2 * U] + hz[:, U:])
                hh = torch.tanh(xp[:, 2 * U:] + (rr * hst) @ r[:, 2 * U:])
                hst = z * hst + (1.0 - z) * hh
            return hst
        finals = [gru_last(w['seq_emb'][i64(q)], 'seq%d_gru' % i) for i, q in enumerate(seqs)]
        cg = gru_last(w['cat_emb'][ids], 'cat_gru')
        feat = torch.cat(finals + [h, cg, w['cat_emb'][ids].reshape(N, -1)], dim=1)
        return elu(feat @ w['obs_w'] + w['obs_b'])
    assert algo == 'dien', algo
    Ec = w['cat_emb'][ids]
    att = torch.softmax(Ec @ Ec.transpose(1, 2), dim=-1) @ Ec
    c = torch.cat([att.mean(dim=1), Ec.reshape(N, -1)], dim=1)
    q = w['seq_emb'][ids[:, -10:]].mean(dim=1)

    def cell(xt, hs, Wg, bg, Wc, bc, a=None):
        n = Wc.shape[1]
        g = sig(torch.cat([xt, hs], dim=1) @ Wg + bg)
        r, u = g[:, :n], g[:, n:]
        cc = torch.tanh(torch.cat([xt, r * hs], dim=1) @ Wc + bc)
        if a is not None:
            u = (1.0 - a) * u
        return u * hs + (1.0 - u) * cc

    finals = []
    for i, sq in enumerate(seqs):
        X = w['seq_emb'][i64(sq)]
        L, E = X.shape[1], X.shape[2]
        hs = torch.zeros((N, E), dtype=torch.float64)
        keys = []
        for t in range(L):
            hs = cell(X[:, t], hs, w['gru%d_gate_w' % i], w['gru%d_gate_b' % i], w['gru%d_cand_w' % i], w['gru%d_cand_b' % i])
            keys.append(hs)
        Kk = torch.stack(keys, dim=1)
        qq = q[:, None, :].expand_as(Kk)
        a = torch.cat([qq, Kk, qq - Kk, qq * Kk], dim=-1)
        s1 = sig(a @ w['att%d_w1' % i] + w['att%d_b1' % i])
        s2 = sig(s1 @ w['att%d_w2' % i] + w['att%d_b2' % i])
        score = (s2 @ w['att%d_w3' % i] + w['att%d_b3' % i])[..., 0]
        h2 = torch.zeros((N, 2 * E), dtype=torch.float64)
        for t in range(L):
            h2 = cell(Kk[:, t], h2, w['augru%d_gate_w' % i], w['augru%d_gate_b' % i], w['augru%d_cand_w' % i],
                      w['augru%d_cand_b' % i], score[:, t:t + 1])
        finals.append(h2)
    allf = torch.cat(finals + [h, c], dim=1)
    return elu(allf @ w['obs_w'] + w['obs_b'])


def head_outputs(torch, head, logits, labels):
    """-> (pred, row losses or None)"""
    if head in ('item', 'multiclass'):
        pred = torch.softmax(logits, dim=1)
    else:
        pred = torch.sigmoid(logits)
    if labels is None:
        return pred, None
    if head == 'item':
        y = torch.nn.functional.one_hot(torch.tensor(np.asarray(labels, dtype=np.int64)), logits.shape[1]).double()
        pc = torch.clamp(pred, 1e-7, 1.0 - 1e-7)
        return pred, -(y * torch.log(pc) + (1.0 - y) * torch.log(1.0 - pc)).mean(dim=1)
    if head == 'multiclass':
        c = torch.tensor(slate_class(labels))
        return pred, torch.logsumexp(logits, dim=1) - logits.gather(1, c[:, None])[:, 0]
    y = torch.tensor((np.asarray(labels) != 0).astype(np.float64))
    bce = (torch.clamp(logits, min=0.0) - logits * y + torch.log1p(torch.exp(-torch.abs(logits)))).mean(dim=1)
    if head == 'slate':
        return pred, bce
    assert head == 'adversarial', head
    return pred, 0.1 * bce + (torch.softmax(pred, dim=1) * (1.0 - y)).sum(dim=1)


def forward(algo, head, weights, cfg, dense, cat, labels, seqs=None, mask1=None, mask2=None, rate=0.0, want_grad=False):
    """-> dict(pred [N, K], loss_rows [N] or None, loss, grads (want_grad)) in float64.  seqs: list of [N, L] id arrays."""
    import torch
    w = dict((k, torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=want_grad)) for k, v in weights.items())
    obs = _trunk(torch, algo, w, cfg, dense, cat, seqs, mask1, mask2, rate)
    logits = obs @ w['out_w'] + w['out_b']
    pred, rows = head_outputs(torch, head, logits, labels)
    out = {'pred': pred.detach().numpy(), 'loss_rows': None if rows is None else rows.detach().numpy(),
           'loss': None if rows is None else float(rows.mean().item())}
    if want_grad:
        rows.mean().backward()
        out['grads'] = dict((k, v.grad.numpy()) for k, v in w.items() if v.grad is not None)
    return out
