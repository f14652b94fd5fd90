"""Restatement of the MDP checker's seq2seq transformer in torch (float64 by default, float32 to measure the format's own error)
and a textbook beam search over it.  DESIGN 33 has the model in words; include/rl4rs_hip.h has the flat parameter layout that
``layout`` repeats here on purpose (a second, independent statement of it).

The model is the published form of keras_transformer.get_model(encoder_num=decoder_num=head_num=1, use_same_embed=False) as
remembered - parity with keras_transformer is unpinned.  ``beam_search_ref`` is pinned: tests/golden/mdp_beam_*.npz hold what the
reference's own beam_search returns for this model (tests/golden/make_mdp_golden.py).
"""
import numpy as np
import torch

PAD, START, END = 0, 1, 2
ATT = ('Wq', 'bq', 'Wk', 'bk', 'Wv', 'bv', 'Wo', 'bo', 'g', 'b')
FFN = ('W1', 'b1', 'W2', 'b2', 'g', 'b')


def layout(V, d, h):
    """[(name, shape)] in flat order; matrices are [in, out]"""
    out = [('E_enc', (V, d)), ('E_dec', (V, d))]

    def att(p):
        return [(p + n, (d, d) if n[0] == 'W' else (d,)) for n in ATT]

    def ffn(p):
        shapes = {'W1': (d, h), 'b1': (h,), 'W2': (h, d), 'b2': (d,), 'g': (d,), 'b': (d,)}
        return [(p + n, shapes[n]) for n in FFN]
    out += att('ea.') + ffn('ef.') + att('ds.') + att('dc.') + ffn('df.')
    out.append(('out_b', (V,)))
    return out


def random_params(V, d, h, seed):
    """Test weights from a RandomState seed: every bias and every layer-norm scale is away from its trivial value, so that a kernel
    that dropped one would show; tables wide enough (std 0.3) for peaked, well-separated output distributions."""
    rs = np.random.RandomState(seed)
    parts = []
    for name, shape in layout(V, d, h):
        leaf = name.split('.')[-1]
        if leaf.startswith('E_'):
            x = rs.normal(0.0, 0.3, shape)
        elif leaf[0] == 'W':
            x = rs.normal(0.0, np.sqrt(2.0 / (shape[0] + shape[1])), shape)
        elif leaf == 'g':
            x = 1.0 + 0.1 * rs.normal(size=shape)
        else:
            x = 0.1 * rs.normal(size=shape)
        parts.append(x.astype(np.float32).ravel())
    return np.concatenate(parts)


M32 = np.uint64(0xffffffff)


def mix32(x):
    """csrc/common.hpp mix32 on uint64 arrays that hold 32-bit values"""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def keep(rate, seed, step, site, rows, cols):
    """keep factors 0 or 1 / (1 - rate): csrc/common.hpp uniform01(seed, step, row, site * 65536 + col) >= rate, in float32"""
    rows, a = np.asarray(rows, dtype=np.uint64), np.uint64(site * 65536) + np.asarray(cols, dtype=np.uint64)
    s_ = mix32((np.uint64(step & 0xffffffff) * np.uint64(0x9E3779B9) + np.uint64(0x85EBCA6B)) & M32)
    r_ = mix32((rows * np.uint64(0xC2B2AE35) + a * np.uint64(0x27D4EB2F) + np.uint64(1)) & M32)
    h_ = mix32((mix32((np.uint64(seed & 0xffffffff) ^ s_ ^ r_) & M32) + a) & M32)
    u = (((h_ >> np.uint64(9)).astype(np.float64) + 0.5) / 8388608.0).astype(np.float32)
    return np.where(u >= np.float32(rate), 1.0 / (1.0 - float(np.float32(rate))), 0.0)


def grad_errors(got, want, V, d, h):
    """per tensor of the layout: max |got - want| / max(max |want| of the tensor, 1e-3 max |want| of the whole gradient) - a tensor
    whose gradient is (almost) nothing, like a key bias, which softmax cancels, is measured against the gradient's overall size"""
    out, o, top = {}, 0, np.abs(want).max()
    for name, shape in layout(V, d, h):
        n = int(np.prod(shape))
        a, b = got[o:o + n], want[o:o + n]
        o += n
        out[name] = np.abs(a - b).max() / max(np.abs(b).max(), 1e-3 * top)
    return out


def pos_table(n, d, dtype):
    j = torch.arange(n, dtype=torch.float64)[:, None]
    c = torch.arange(d)[None, :]
    ang = j / torch.pow(torch.tensor(10000.0, dtype=torch.float64), (2 * (c // 2)).to(torch.float64) / d)
    return torch.where(c % 2 == 0, torch.sin(ang), torch.cos(ang)).to(dtype)


class RefSeq2Seq:
    def __init__(self, V, d, h, flat, dtype=torch.float64):
        self.V, self.d, self.h, self.dtype = V, d, h, dtype
        self.p = {}
        o = 0
        flat = np.asarray(flat, dtype=np.float32)
        for name, shape in layout(V, d, h):
            n = int(np.prod(shape))
            self.p[name] = torch.from_numpy(flat[o:o + n].reshape(shape).copy()).to(dtype)
            o += n
        assert o == flat.size, (o, flat.size)
        self.pos = pos_table(64, d, dtype)

    SITES = {'ea.': 0, 'ef.': 1, 'ds.': 2, 'dc.': 3, 'df.': 4}
    drop = None                                  # (rate, seed, step) while a training forward runs

    def _drop(self, y, pre):
        """the library's keep factors on a block's [N, L, d] sub-layer output: row = n * L + l, col = feature, one site per block"""
        if self.drop is None or self.drop[0] <= 0:
            return y
        N, L, d = y.shape
        k = keep(self.drop[0], self.drop[1], self.drop[2], self.SITES[pre], np.arange(N * L).reshape(N * L, 1), np.arange(d).reshape(1, d))
        return y * torch.from_numpy(k.reshape(N, L, d)).to(self.dtype)

    def loss_and_grad(self, enc, dec_in, dec_out, drop=None):
        """masked cross-entropy (mean over the positions whose decoder INPUT is not PAD) and autograd's gradient, flat, in layout order"""
        names = [n for n, _ in layout(self.V, self.d, self.h)]
        for n in names:
            self.p[n] = self.p[n].detach().requires_grad_(True)
        self.drop = drop
        try:
            pr = self.forward(enc, dec_in)
        finally:
            self.drop = None
        tgt = torch.as_tensor(np.asarray(dec_out), dtype=torch.long)
        w = torch.as_tensor(np.asarray(dec_in) != PAD).to(self.dtype)
        nll = -torch.log(torch.gather(pr, 2, tgt[:, :, None])[:, :, 0])
        loss = (nll * w).sum() / w.sum()
        grads = torch.autograd.grad(loss, [self.p[n] for n in names])
        for n in names:
            self.p[n] = self.p[n].detach()
        return float(loss.detach()), np.concatenate([g.detach().numpy().ravel() for g in grads])

    def _ln(self, x, pre):
        mean = x.mean(-1, keepdim=True)
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
        return self.p[pre + 'g'] * ((x - mean) / torch.sqrt(var + 1e-14)) + self.p[pre + 'b']

    def _att(self, pre, xq, xkv, key_open, causal):
        p = self.p
        q = xq @ p[pre + 'Wq'] + p[pre + 'bq']
        k = xkv @ p[pre + 'Wk'] + p[pre + 'bk']
        v = xkv @ p[pre + 'Wv'] + p[pre + 'bv']
        s = q @ k.transpose(1, 2) / np.sqrt(self.d)
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        mask = key_open[:, None, :].to(self.dtype)
        if causal:
            L = xq.shape[1]
            mask = mask * torch.tril(torch.ones(L, L, dtype=self.dtype))[None]
        e = e * mask
        a = e / (e.sum(-1, keepdim=True) + 1e-7)
        return self._ln(xq + self._drop((a @ v) @ p[pre + 'Wo'] + p[pre + 'bo'], pre), pre)

    def _ffn(self, pre, x):
        p = self.p
        f = torch.relu(x @ p[pre + 'W1'] + p[pre + 'b1']) @ p[pre + 'W2'] + p[pre + 'b2']
        return self._ln(x + self._drop(f, pre), pre)

    def forward(self, enc, dec):
        """enc int [N, S], dec int [N, L] -> probabilities [N, L, V] (torch, self.dtype)"""
        enc = torch.as_tensor(np.asarray(enc), dtype=torch.long)
        dec = torch.as_tensor(np.asarray(dec), dtype=torch.long)
        S, L = enc.shape[1], dec.shape[1]
        x = self.p['E_enc'][enc] + self.pos[:S][None]
        x = self._ffn('ef.', self._att('ea.', x, x, enc != PAD, False))
        y = self.p['E_dec'][dec] + self.pos[:L][None]
        y = self._att('ds.', y, y, dec != PAD, True)
        y = self._att('dc.', y, x, enc != PAD, False)
        y = self._ffn('df.', y)
        return torch.softmax(y @ self.p['E_dec'].t() + self.p['out_b'], dim=-1)

    def predict(self, xs):
        """keras' model.predict([enc, dec]) for the reference's decoder functions"""
        with torch.no_grad():
            return self.forward(xs[0], xs[1]).numpy()


def adam_ref(params, grads_fn, steps, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """Keras 'adam' in float64: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), p -= lr_t m / (sqrt(v) + eps); grads_fn(params) -> gradient"""
    p = np.asarray(params, dtype=np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, steps + 1):
        g = np.asarray(grads_fn(p), dtype=np.float64)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps)
    return p


def adam_f32(params, grads_fn, steps, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """the same optimiser with parameters, moments and arithmetic in float32 (lr_t formed in float64 and cast, as the library forms
    it): what the number format alone does to adam_ref.  grads_fn(float32 params) -> gradient"""
    f = np.float32
    p = np.asarray(params, dtype=f).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, steps + 1):
        g = np.asarray(grads_fn(p), dtype=f)
        m = f(b1) * m + (f(1) - f(b1)) * g
        v = f(b2) * v + (f(1) - f(b2)) * g * g
        p = p - f(lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)) * m / (np.sqrt(v) + f(eps))
    return p


ADAM_STEPS = 3


def adam_check(step_fn):
    """Three Adam steps on FORWARD_CASES[0] without dropout.  step_fn(V, d, h, flat, enc, dec_in, dec_out, steps) -> parameters.
    -> the largest |parameters - adam_ref's| over the FIRM elements, those whose first float64 gradient exceeds 1e-3 of the
    gradient's largest element.  The first steps move an element by about lr whatever its gradient's size (m / sqrt(v) is +-1), so
    where the gradient is within rounding of zero the direction of the move is rounding too: such elements say nothing."""
    V, d, h, flat, enc, dec = forward_case(0)
    out = train_targets(0)
    first = []

    def grad64(p):
        g = RefSeq2Seq(V, d, h, p.astype(np.float32)).loss_and_grad(enc, dec, out)[1]
        first.append(g)
        return g
    want = adam_ref(flat, grad64, ADAM_STEPS)
    assert np.abs(want - flat).max() > 2.5e-3                    # three steps of about lr each
    firm = np.abs(first[0]) > 1e-3 * np.abs(first[0]).max()
    assert firm.mean() > 0.3
    got = np.asarray(step_fn(V, d, h, flat, enc, dec, out, ADAM_STEPS), dtype=np.float64)
    return np.abs(got - want)[firm].max()


def beam_search_ref(model, enc, K, T, candidates_size=None):
    """Textbook beam search on products of probabilities in float64, equal scores by the smaller beam * V + token.
    -> paths int64 [N, K, T + 1], scores float64 [N, K], step_probs float64 [N, K, T], margin float64 [N]: the smallest relative gap
    between adjacent kept candidates (last kept vs first dropped included) over all steps, and, with candidates, between the last
    token inside the candidate set and the first outside it."""
    enc = np.asarray(enc)
    N, V = enc.shape[0], model.V
    paths = np.zeros((N, 1, T + 1), dtype=np.int64)
    paths[:, :, 0] = START
    scores = np.ones((N, 1))
    sp = np.zeros((N, 1, T))
    margin = np.full(N, np.inf)
    cand_mask = None
    for t in range(T):
        live = paths.shape[1]
        # one prediction per live beam on the N users, as the reference batches them (a batched product of another shape may
        # round its float64 sums in another order, and the golden scores are compared exactly)
        pr = np.stack([model.predict([enc, paths[:, b, :t + 1]])[:, -1].astype(np.float64) for b in range(live)], axis=1)
        if t == 0 and candidates_size is not None:
            order = np.argsort(-pr[:, 0], axis=1, kind='stable')
            cand_mask = np.zeros((N, V))
            np.put_along_axis(cand_mask, order[:, :candidates_size], 1.0, axis=1)
            top = np.take_along_axis(pr[:, 0], order, axis=1)
            if candidates_size < V:
                margin = np.minimum(margin, (top[:, candidates_size - 1] - top[:, candidates_size]) / top[:, candidates_size - 1])
        if t > 0 and cand_mask is not None:
            pr = pr * cand_mask[:, None, :]
        total = (scores[:, :, None] * pr).reshape(N, live * V)
        order = np.argsort(-total, axis=1, kind='stable')[:, :K + 1]
        val = np.take_along_axis(total, order, axis=1)
        with np.errstate(divide='ignore', invalid='ignore'):
            gaps = (val[:, :K] - val[:, 1:K + 1]) / val[:, :K]
        margin = np.minimum(margin, np.nan_to_num(gaps, nan=0.0).min(axis=1))
        order, val = order[:, :K], val[:, :K]
        par, tok = order // V, order % V
        new_paths = np.take_along_axis(paths, par[:, :, None], axis=1).copy()
        new_paths[:, :, t + 1] = tok
        new_sp = np.take_along_axis(sp, par[:, :, None], axis=1).copy()
        new_sp[:, :, t] = pr.reshape(N, live * V)[np.arange(N)[:, None], order]
        paths, scores, sp = new_paths, val, new_sp
    return paths, scores, sp, margin



# ---------------------------------------------------------------- the learning check
LEARN = dict(V=40, d=64, h=48, src_items=4, T=3, train=2048, held=512, batch=256, rate=0.05, seed=3)
# `python tests/mdp_ref.py learn` (CPU): the restatement, trained as Seq2SeqTransformer.fit trains (same initial parameters, batches,
# dropout masks, float64 Keras Adam), first decodes >= 95 % of the held-out targets exactly under greedy search after LEARN_EPOCHS
# epochs, at LEARN_RATE
LEARN_EPOCHS, LEARN_RATE = 28, 0.98828125      # epochs 25 .. 28: 0.4355, 0.6895, 0.9141, 0.9883 (506 of 512)


def learn_data():
    """a deterministic MDP: target token j (1-based) = (last source item + j) mod 37 + 3; script framing of both sides"""
    c = LEARN
    rs = np.random.RandomState(c['seed'])
    n = c['train'] + c['held']
    items = rs.randint(3, c['V'], size=(n, c['src_items']))
    tgt = (items[:, -1:] + np.arange(1, c['T'] + 1)[None]) % 37 + 3
    one = np.ones((n, 1), dtype=np.int64)
    enc = np.concatenate([one * START, items, one * END], axis=1).astype(np.int32)
    dec_in = np.concatenate([one * START, tgt, one * END], axis=1).astype(np.int32)
    dec_out = np.concatenate([tgt, one * END, one * PAD], axis=1).astype(np.int32)
    return enc, dec_in, dec_out, tgt


def greedy_ref(model, enc, T):
    paths = np.full((len(enc), 1), START, dtype=np.int64)
    for _ in range(T):
        paths = np.concatenate([paths, model.predict([enc, paths])[:, -1].argmax(axis=1)[:, None]], axis=1)
    return paths[:, 1:]


def train_ref(flat, epochs, on_epoch):
    """Seq2SeqTransformer.fit restated: epoch e shuffles with RandomState(seed * 1000003 + e), batch b of the run draws the masks of
    (seed, b); float64 Keras Adam.  on_epoch(e, params) -> True stops."""
    c = LEARN
    enc, dec_in, dec_out, _ = learn_data()
    enc, dec_in, dec_out = enc[:c['train']], dec_in[:c['train']], dec_out[:c['train']]
    p = np.asarray(flat, dtype=np.float64).copy()
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    for e in range(epochs):
        order = np.random.RandomState(c['seed'] * 1000003 + e).permutation(c['train'])
        for a in range(0, c['train'], c['batch']):
            idx = order[a:a + c['batch']]
            g = RefSeq2Seq(c['V'], c['d'], c['h'], p.astype(np.float32)).loss_and_grad(enc[idx], dec_in[idx], dec_out[idx], (c['rate'], c['seed'], t))[1]
            t += 1
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            p = p - 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (np.sqrt(v) + 1e-7)
        if on_epoch(e + 1, p):
            break
    return p


# ---------------------------------------------------------------- shared cases and error bars
GOLDEN_CASES = ('n3_v37_k4', 'n70_v37_k8', 'n4_v37_k1', 'n3_v50_k6_c9', 'n2_v290_k100', 'n2_v290_k20_c20')
# (N, src_len, L, V, d, hidden): the two shapes the forward is specified at and one whose row counts (45 * 18, 45 * 6) are no
# multiple of a GEMM tile; every case has PAD keys in a source and in a decoder input, the L = 1 call is cut from the first
FORWARD_CASES = ((5, 18, 7, 37, 64, 48), (3, 5, 3, 290, 256, 128), (45, 18, 6, 37, 64, 48))

# Error bars = 4 x the float32 error of this restatement against itself in float64 at the very inputs of the tests, measured on a
# CPU by `python tests/mdp_ref.py` (per width d; the measured maxima are in the comments).  Never taken from the kernels.
FWD_ABS_BAR = {64: 4 * 6.6e-7, 256: 4 * 9.6e-7}      # |p32 - p64|:                64: 6.51e-7 (45 x 18 x 6 case), 256: 9.51e-7
FWD_REL_BAR = {64: 4 * 4.5e-6, 256: 4 * 1.25e-5}     # |p32 - p64| / p64, p > 1e-6: 64: 4.44e-6,                  256: 1.25e-5
BEAM_REL_BAR = {64: 4 * 3.0e-6, 256: 4 * 8.2e-6}     # beam scores, relative:       64: 2.96e-6 (n70_v37_k8),     256: 8.18e-6 (n2_v290_k100)

# the training pass at FORWARD_CASES[0] and [1] (train_targets), dropout 0 and 0.05 at (seed 7, step 3): loss relative, and
# grad_errors per tensor (worst: a key bias).  64: 1.06e-7, 2.14e-6; 256: 1.83e-7, 3.37e-6
# adam_check with adam_f32 on the float32 restatement's gradients: 1.69e-7
ADAM_BAR = 4 * 1.7e-7
LOSS_REL_BAR = {64: 4 * 1.1e-7, 256: 4 * 1.9e-7}
GRAD_BAR = {64: 4 * 2.2e-6, 256: 4 * 3.4e-6}


def _tokens_with_pad(shape, seed):
    N, S, L, V, d, h = shape
    rs = np.random.RandomState(seed)
    enc = rs.randint(1, V, size=(N, S)).astype(np.int32)
    dec = rs.randint(1, V, size=(N, L)).astype(np.int32)
    dec[:, 0] = START
    enc[0, -2:] = PAD
    dec[1, -1] = PAD
    if L > 2:
        dec[2, 1] = PAD              # a PAD key in front of later queries
    return enc, dec


def _targets(dec, V, seed):
    out = np.random.RandomState(seed).randint(1, V, size=dec.shape).astype(np.int32)
    out[:, :-1] = np.where(dec[:, 1:] != PAD, dec[:, 1:], out[:, :-1])
    return out


def forward_case(i):
    """-> (V, d, h, flat parameters, enc [N, S], dec [N, L]) of FORWARD_CASES[i]"""
    N, S, L, V, d, h = FORWARD_CASES[i]
    enc, dec = _tokens_with_pad(FORWARD_CASES[i], 50 + i)
    return V, d, h, random_params(V, d, h, 3 + i), enc, dec


def train_targets(i):
    """decoder outputs [N, L] for forward_case(i): the inputs shifted by one, PAD where the input is PAD's successor"""
    return _targets(forward_case(i)[5], FORWARD_CASES[i][3], 70 + i)


# ---------------------------------------------------------------- off the two default shapes (tests/test_gpu_mdp_shapes.py)
# (N, src_len, L, V, d, hidden), each with the path of csrc/seq2seq.hip, seq2seq_train.hpp and gemm.hip it enters.  launch_gemm_f32
# has three forms: k_gemm_small below 96 workgroups of 128 x 64 (or N <= 32), k_gemm_f32_t128 from 2048 rows with N >= 96 and every
# size and pointer a multiple of 4 floats, k_gemm_f32 otherwise.  With d = 128 a d-wide product has two column tiles, so it leaves
# k_gemm_small only from 6017 rows; the tied output layer at V = 292 has five and leaves it from 2433 rows.  Cases 9 and 10 are
# sized by that: they, not 6 .. 8, reach the two large forms.
SHAPE_CASES = (
    # 0: every lane of a wave is a key, in both self-attentions and in cross-attention; the causal mask at 64 queries
    (3, 64, 64, 37, 64, 48),
    # 1: L > S: k_s2s_attn_bwd_kv of the cross-attention loops over more queries than there are keys, max_rows = N * L
    (4, 3, 9, 37, 64, 48),
    # 2: one key, one query, in training too; user 0's only source token and user 1's only decoder input are PAD
    (5, 1, 1, 37, 64, 48),
    # 3: d % 4 == 2: the tail guard of every per-row kernel is live in the second 64-stride, no row of an activation is 16-byte
    #    aligned (scalar loads in every GEMM); odd hidden width: every matrix behind ef.b1 lies off 16-byte alignment
    (5, 7, 5, 41, 66, 7),
    # 4: d % 64 != 0 with d % 4 == 0: tail guard live, vector loads stay; carries dropout 0.5
    (5, 7, 5, 41, 100, 33),
    # 5: the narrowest widths s2s_check_cfg admits, but for d = 2 and 4 (there a row is one pair of position columns)
    (5, 7, 5, 41, 6, 1),
    # 6: 2304 encoder rows: s2s_chunk = 256 with 9 partials in every encoder weight gradient, 18 row tiles per GEMM (k_gemm_small:
    #    36 workgroups), strided KV + D outputs (ldc = 2 d) at many rows
    (36, 64, 8, 292, 128, 100),
    # 7: the same rows with hidden % 4 == 2: every matrix behind ef.b1 off 16-byte alignment (scalar weight loads in k_gemm_nt)
    (36, 64, 8, 292, 128, 102),
    # 8: 4480 encoder rows: s2s_chunk = ceil(4480 / 16) = 280, no multiple of the 16-sample trip of k_gemm_tn, 16 partials; 2310
    #    decoder rows through the tied output layer (ldw = Vp) and its weight gradient: 19 x 5 = 95 workgroups, the last k_gemm_small
    (70, 64, 33, 292, 128, 100),
    # 9: 6080 encoder rows: 48 x 2 = 96 workgroups, so every d-wide projection of the encoder (N = 128) and its FFN (N = 100) run
    #    k_gemm_f32_t128, with the strided KV + D outputs; 2470 decoder rows: 20 x 5 = 100, the tied output layer (N = 292, ldw = Vp)
    #    runs it too; s2s_chunk = 380
    (95, 64, 26, 292, 128, 100),
    # 10: the same rows with hidden % 4 == 2: ef.W1 (N = 102) and everything behind it, off alignment, run k_gemm_f32; the encoder
    #    attention's projections and the output layer (the transposed table is a buffer of its own) stay in k_gemm_f32_t128
    (95, 64, 26, 292, 128, 102),
)
SHAPE_DROP = (0.05, 7, 3)
SHAPE_DROP_HALF = {4: (0.5, 7, 3)}               # case -> a second dropout setting

# Per case: 4 x what `python tests/mdp_ref.py shapes` prints (the float32 restatement against float64 at the case's own inputs; for
# the loss and the gradient the largest of the case's dropout settings).  The measured maxima stand in the comments.  A figure
# below float32's unit roundoff 2^-24 is luck, not a property of the format - the loss is ONE float32 number, and a probability near
# 1 cannot be stored closer than that - so a measured figure counts as at least F32_ROUND.  Never taken from the kernels.
F32_ROUND = 6.0e-8


def _bars(p_abs, p_rel, loss, grad):
    return dict(abs=4 * max(p_abs, F32_ROUND), rel=4 * p_rel, loss=4 * max(loss, F32_ROUND), grad=4 * grad)


SHAPE_BARS = {                                   # |p32 - p64|, the same / p64 where p > 1e-6, loss relative, worst grad_errors tensor
    0: _bars(7.2e-7, 4.3e-6, 8.4e-8, 3.1e-6),    # 7.13e-7  4.24e-6  8.35e-8  3.00e-6 (dc.bk)
    1: _bars(5.0e-7, 3.2e-6, 4.7e-8, 4.4e-6),    # 4.99e-7  3.14e-6  4.67e-8  4.31e-6 (dc.bk)
    2: _bars(5.7e-7, 2.6e-6, 3.2e-8, 1.2e-6),    # 5.62e-7  2.56e-6  3.20e-8  1.11e-6 (E_dec)
    3: _bars(4.6e-7, 4.4e-6, 1.0e-7, 3.1e-6),    # 4.52e-7  4.35e-6  9.93e-8  3.08e-6 (dc.bk)
    4: _bars(6.8e-7, 4.6e-6, 5.5e-8, 4.6e-6),    # 6.74e-7  4.55e-6  5.48e-8  4.59e-6 (dc.bk)
    5: _bars(2.2e-8, 3.8e-7, 2.9e-8, 9.1e-6),    # 2.14e-8  3.78e-7  2.84e-8  9.07e-6 (ef.b1)
    6: _bars(1.8e-6, 8.6e-6, 3.6e-8, 1.1e-6),    # 1.73e-6  8.53e-6  3.52e-8  1.00e-6 (ea.bk)
    7: _bars(2.0e-6, 1.2e-5, 5.2e-8, 1.6e-6),    # 1.93e-6  1.19e-5  5.15e-8  1.55e-6 (ds.Wq)
    8: _bars(1.7e-6, 1.1e-5, 6.8e-8, 9.2e-7),    # 1.64e-6  1.03e-5  6.74e-8  9.18e-7 (ds.Wq)
    9: _bars(2.3e-6, 1.2e-5, 8.8e-8, 5.4e-7),    # 2.24e-6  1.14e-5  8.78e-8  5.37e-7 (ds.Wv)
    10: _bars(2.1e-6, 1.1e-5, 1.1e-7, 6.3e-7),   # 2.00e-6  1.08e-5  1.00e-7  6.22e-7 (ds.Wq)
}


def shape_case(i):
    """-> (V, d, h, flat parameters, enc [N, S], dec [N, L]) of SHAPE_CASES[i], PAD keys placed as forward_case places them"""
    N, S, L, V, d, h = SHAPE_CASES[i]
    enc, dec = _tokens_with_pad(SHAPE_CASES[i], 150 + i)
    return V, d, h, random_params(V, d, h, 30 + i), enc, dec


def shape_targets(i):
    return _targets(shape_case(i)[5], SHAPE_CASES[i][3], 170 + i)


def shape_drops(i):
    return [None, SHAPE_DROP] + ([SHAPE_DROP_HALF[i]] if i in SHAPE_DROP_HALF else [])


def masked_rows_case():
    """FORWARD_CASES[0] with user 3's source all PAD and user 4's decoder input all PAD behind <START>
    -> (V, d, h, flat, enc, dec, targets, lost): lost = the tokens that only user 3's source held"""
    V, d, h, flat, enc, dec = forward_case(0)
    enc, dec = enc.copy(), dec.copy()
    others = np.delete(enc, 3, axis=0)
    lost = sorted(int(v) for v in set(enc[3].tolist()) if not (others == v).any())
    enc[3] = PAD
    dec[4, 1:] = PAD
    return V, d, h, flat, enc, dec, _targets(dec, V, 70), lost


def masked_max_case(causal=False):
    """Masked keys that tower over the open ones, so that sum e comes near the normaliser's 1e-7 and the max-shift term of the
    attention's reverse pass carries weight: ea and ds score by q . k of the bare inputs (Wq = Wk = 1, the biases stay), column
    d - 1 of both tables is 3 for every token and 25 for PAD (the position table adds about 1 there), so for an open query a PAD key
    outscores an open key by about 4 * (26 - 4) / sqrt(64) = 11 before the max.  causal: the towering key is token 9 instead of PAD,
    in the last but one decoder position - future, under the causal mask, for all queries before it - and PAD is placed as
    forward_case places it.  -> (V, d, h, flat, enc, dec, targets)"""
    V, d, h = 37, 64, 48
    flat = random_params(V, d, h, 27).copy()
    o = 0
    at = {}
    for name, shape in layout(V, d, h):
        at[name] = (o, shape)
        o += int(np.prod(shape))
    for name in ('ea.Wq', 'ea.Wk', 'ds.Wq', 'ds.Wk'):
        flat[at[name][0]:at[name][0] + d * d] = np.eye(d, dtype=np.float32).ravel()
    for name in ('E_enc', 'E_dec'):
        E = flat[at[name][0]:at[name][0] + V * d].reshape(V, d)        # a view: writes go to flat
        E[:, d - 1] = 3.0
        E[9 if causal else PAD, d - 1] = 25.0
    N, S, L = 5, 18, 7
    rs = np.random.RandomState(28)
    enc = rs.randint(1, V, size=(N, S)).astype(np.int32)
    dec = rs.randint(1, V, size=(N, L)).astype(np.int32)
    dec[:, 0] = START
    if causal:
        enc[enc == 9] = 10
        dec[dec == 9] = 10
        dec[:, L - 2] = 9                        # future for the queries 0 .. L - 3
        enc[0, -2:] = PAD
        dec[1, -1] = PAD
    else:
        enc[:, 1::3] = PAD
        dec[:, 2::3] = PAD
    return V, d, h, flat, enc, dec, _targets(dec, V, 29)


MASKED_ROWS_BARS = _bars(4.6e-7, 4.1e-6, 1.8e-8, 1.9e-6)            # 4.59e-7  4.04e-6  1.75e-8  1.82e-6 (ds.bk); dropout 0 and SHAPE_DROP
# (the probabilities of the masked-max cases are not compared: PAD's output logit towers too, the rest is below 1e-6)
MASKED_MAX_BARS = {False: _bars(0, 0, 5.5e-8, 2.2e-6),              # loss 5.49e-8, gradient 2.19e-6 (ds.Wk)
                   True: _bars(0, 0, 1.5e-8, 6.1e-6)}               # loss 1.49e-8, gradient 6.02e-6 (ds.Wq)


# beam-search edges: (N, S, V, K, T, candidates_size, seed); weights random_params(V, 64, 48, seed), sources
# RandomState(seed + 1).randint(3, V) between <START> and <END>
BEAM_CASES = (
    # 0: beam 64, the last width at which one list head per lane suffices in k_s2s_merge
    (4, 6, 70, 64, 3, None, 12),
    # 1: beam 65, the first width at which lane 0 keeps a second head
    (4, 6, 70, 65, 3, None, 12),
    # 2: the same under candidate sets of beam + 3 tokens: all but 3 of a row's V - 65 unkept items are zero products, which tie
    (4, 6, 70, 65, 3, 68, 12),
    # 3: S2S_BEAM_MAX with V = beam + 1, the smallest vocabulary `beam < token_num` admits: a row's list drops one token
    (8, 6, 129, 128, 3, None, 19),
    # 4: target_len 63: T1 = 64, the stride the prefix and sp buffers are allocated with; table attention over up to 63 prefix keys
    (4, 6, 37, 4, 63, None, 13),
    # 5: 2400 beam rows, V % 4 == 0: 19 x 5 = 95 workgroups, the output layer's last k_gemm_small
    (24, 6, 292, 100, 3, None, 14),
    # 6: 2500 beam rows: 20 x 5 = 100 workgroups, the output layer runs k_gemm_f32_t128 (ldw = Vp); candidate sets of beam + 4
    (25, 6, 292, 100, 3, 104, 14),
)
# 4 x the float32 search's scores against the float64 search's, relative; the share of users whose every float64 selection margin
# exceeds that bar is 0.75, 0.75, 0.75, 0.875, 1, 0.83, 0.84 (tests/test_mdp_host.py asserts >= 0.75)
BEAM_BARS = {0: 4 * 3.9e-6, 1: 4 * 3.9e-6, 2: 4 * 3.9e-6,           # 3.89e-6 each
             3: 4 * 3.9e-6,                                          # 3.85e-6
             4: 4 * 3.8e-6,                                          # 3.78e-6; the smallest score is 2.5e-5
             5: 4 * 4.7e-6, 6: 4 * 4.7e-6}                           # 4.60e-6 each


def beam_case(i):
    N, S, V, K, T, Cn, seed = BEAM_CASES[i]
    d, h = 64, 48
    enc = np.random.RandomState(seed + 1).randint(3, V, size=(N, S)).astype(np.int32)
    enc[:, 0], enc[:, -1] = START, END
    return dict(N=N, S=S, V=V, K=K, T=T, C=Cn, d=d, h=h, seed=seed, enc=enc, flat=random_params(V, d, h, seed))


def load_case(golden_dir, name):
    import os
    z = np.load(os.path.join(golden_dir, 'mdp_beam_%s.npz' % name))
    N, V, K, Cn, S, T, d, h, seed = (int(v) for v in z['cfg'])
    return dict(N=N, V=V, K=K, C=Cn or None, S=S, T=T, d=d, h=h, seed=seed, enc=z['encode_input'], paths=z['output_topk'].astype(np.int64),
                scores=z['beam_score'], flat=random_params(V, d, h, seed))


def probs_errors(got, want):
    """-> (max |got - want|, max |got - want| / want where want > 1e-6)"""
    err = np.abs(got - want)
    big = want > 1e-6
    return float(err.max()), float((err[big] / want[big]).max())


def train_errors(V, d, h, flat, enc, dec, out, drops):
    """float32 restatement against float64 -> (loss relative, worst grad_errors figure, its tensor), the largest over `drops`"""
    loss, grad, name = 0.0, 0.0, None
    for drop in drops:
        l64, g64 = RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, out, drop)
        l32, g32 = RefSeq2Seq(V, d, h, flat, torch.float32).loss_and_grad(enc, dec, out, drop)
        e = grad_errors(g32, g64, V, d, h)
        loss = max(loss, abs(l32 - l64) / l64)
        if max(e.values()) > grad:
            grad, name = max(e.values()), max(e, key=e.get)
    return loss, grad, name


def measure_shapes():
    """the figures behind SHAPE_BARS, MASKED_ROWS_BARS, MASKED_MAX_BARS and BEAM_BARS"""
    def one(tag, V, d, h, flat, enc, dec, out, drops):
        a = RefSeq2Seq(V, d, h, flat).predict([enc, dec])
        b = RefSeq2Seq(V, d, h, flat, torch.float32).predict([enc, dec])
        loss, grad, name = train_errors(V, d, h, flat, enc, dec, out, drops)
        print(tag, 'abs %.3g rel (p > 1e-6) %.3g loss rel %.3g grad %.3g (%s)' % (probs_errors(b, a) + (loss, grad, name)), flush=True)
    for i, shape in enumerate(SHAPE_CASES):
        one('shape %d %s' % (i, shape), *shape_case(i), shape_targets(i), shape_drops(i))
    one('masked rows', *masked_rows_case()[:7], [None, SHAPE_DROP])
    one('masked max', *masked_max_case(), [None])
    one('masked max, causal', *masked_max_case(True), [None])
    for i, shape in enumerate(BEAM_CASES):
        c = beam_case(i)
        _, s64, _, margin = beam_search_ref(RefSeq2Seq(c['V'], c['d'], c['h'], c['flat']), c['enc'], c['K'], c['T'], c['C'])
        _, s32, _, _ = beam_search_ref(RefSeq2Seq(c['V'], c['d'], c['h'], c['flat'], torch.float32), c['enc'], c['K'], c['T'], c['C'])
        rel = (np.abs(s32 - s64) / s64).max()
        print('beam %d %s' % (i, shape), 'score rel %.3g' % rel, 'clear share at 4 x that %.3f' % (margin > 4 * rel).mean(),
              'smallest score %.3g' % s64.min(), flush=True)


if __name__ == '__main__':
    import os
    import sys
    if sys.argv[1:] == ['learn']:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from rl4rs_amd.mdpchecker import init_params
        c = LEARN
        enc, _, _, tgt = learn_data()

        def report(e, p):
            got = greedy_ref(RefSeq2Seq(c['V'], c['d'], c['h'], p.astype(np.float32)), enc[c['train']:], c['T'])
            rate = float((got == tgt[c['train']:]).all(axis=1).mean())
            print('epoch %d exact-match %.4f' % (e, rate), flush=True)
            return rate >= 0.95
        train_ref(init_params(c['V'], c['d'], c['h'], c['seed']), 200, report)
        sys.exit(0)
    if sys.argv[1:] in ([], ['shapes']):
        measure_shapes()
    if sys.argv[1:] == ['shapes']:
        sys.exit(0)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    for i, shape in enumerate(FORWARD_CASES):
        V, d, h, flat, enc, dec = forward_case(i)
        a = RefSeq2Seq(V, d, h, flat).predict([enc, dec])
        b = RefSeq2Seq(V, d, h, flat, torch.float32).predict([enc, dec])
        big = a > 1e-6
        print('forward', shape, 'abs %.3g' % np.abs(a - b).max(), 'rel (p > 1e-6) %.3g' % (np.abs(a - b)[big] / a[big]).max())
    for name in GOLDEN_CASES:
        c = load_case(golden, name)
        _, s64, _, margin = beam_search_ref(RefSeq2Seq(c['V'], c['d'], c['h'], c['flat']), c['enc'], c['K'], c['T'], c['C'])
        _, s32, _, _ = beam_search_ref(RefSeq2Seq(c['V'], c['d'], c['h'], c['flat'], torch.float32), c['enc'], c['K'], c['T'], c['C'])
        print('beam', name, 'score rel %.3g' % (np.abs(s32 - s64) / s64).max(), 'smallest margins', np.sort(margin)[:3])
    for i in (0, 1):
        V, d, h, flat, enc, dec = forward_case(i)
        for drop in (None, (0.05, 7, 3)):
            l64, g64 = RefSeq2Seq(V, d, h, flat).loss_and_grad(enc, dec, train_targets(i), drop)
            l32, g32 = RefSeq2Seq(V, d, h, flat, torch.float32).loss_and_grad(enc, dec, train_targets(i), drop)
            e = grad_errors(g32, g64, V, d, h)
            print('train', FORWARD_CASES[i], drop, 'loss rel %.3g' % (abs(l32 - l64) / l64), 'worst tensor', max(e, key=e.get), '%.3g' % max(e.values()))
    print('adam', 'firm elements, float32 against float64 %.3g' % adam_check(
        lambda V, d, h, flat, enc, dec, out, steps: adam_f32(
            flat, lambda p: RefSeq2Seq(V, d, h, p, torch.float32).loss_and_grad(enc, dec, out)[1], steps)))
