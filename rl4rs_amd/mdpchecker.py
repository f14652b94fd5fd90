"""The MDP checker ("data understanding tool") of the reference on the device: the seq2seq transformer it decodes with
(script/mdpchecker/mdp_checker.py:93-102), the beam search of rl4rs/mdpchecker/decoder.py, the script's dataset windowing and the
quantities its two experiments print.

    from rl4rs_amd.mdpchecker import Seq2SeqTransformer, build_dataset, check
    data = build_dataset(open('rl4rs.csv').read().split('\\n')[1:-1], 'rl4rs')
    model = Seq2SeqTransformer(token_num=data['token_num'])
    model.fit([data['encode_input'][:-10000], data['decode_input'][:-10000]], data['decode_output'][:-10000])
    result = check(model, data['encode_input'], name='rl4rs')

The model runs through ``rl4rs_seq2seq_*`` (include/rl4rs_hip.h): ``fit`` (masked cross-entropy, hand-written backward, Keras-form
Adam), ``predict`` and the beam search; ``run(name, dataset_dir)`` is the script end to end.  keras_transformer is not available: the model is its published form as
restated in DESIGN 33, parity unpinned.  ``beam_search`` is pinned to the reference's own function (tests/golden/mdp_beam_*.npz).
There is no CPU path: a model that is not a ``Seq2SeqTransformer`` is a TypeError, a missing device an error.
"""
import random

import numpy as np
import torch

from . import device as D

PAD, START, END = 0, 1, 2
_ATT = ('Wq', 'bq', 'Wk', 'bk', 'Wv', 'bv', 'Wo', 'bo', 'ln_gamma', 'ln_beta')
_FFN = ('W1', 'b1', 'W2', 'b2', 'ln_gamma', 'ln_beta')


def param_layout(token_num, embed_dim, hidden_dim):
    """[(name, shape)] of the flat float32 parameter vector (include/rl4rs_hip.h), matrices [in, out]"""
    V, d, h = int(token_num), int(embed_dim), int(hidden_dim)
    out = [('encoder_embedding', (V, d)), ('decoder_embedding', (V, d))]
    ffn = {'W1': (d, h), 'b1': (h,), 'W2': (h, d), 'b2': (d,), 'ln_gamma': (d,), 'ln_beta': (d,)}
    for block, names in (('encoder_attention', _ATT), ('encoder_ffn', _FFN), ('decoder_self_attention', _ATT),
                         ('decoder_cross_attention', _ATT), ('decoder_ffn', _FFN)):
        for n in names:
            shape = ffn[n] if names is _FFN else ((d, d) if n[0] == 'W' else (d,))
            out.append((block + '/' + n, shape))
    out.append(('output_bias', (V,)))
    return out


def init_params(token_num, embed_dim, hidden_dim, seed=0):
    """keras' defaults: Glorot-normal matrices (truncated at two standard deviations), zero biases, layer norm at (1, 0),
    uniform(-0.05, 0.05) tables"""
    rs = np.random.RandomState(seed)
    parts = []
    for name, shape in param_layout(token_num, embed_dim, hidden_dim):
        leaf = name.split('/')[-1]
        if leaf.endswith('embedding'):
            x = rs.uniform(-0.05, 0.05, shape)
        elif leaf[0] == 'W':
            std = np.sqrt(2.0 / (shape[0] + shape[1])) / 0.87962566103423978
            x = rs.normal(size=shape)
            while True:
                bad = np.abs(x) > 2.0
                if not bad.any():
                    break
                x[bad] = rs.normal(size=int(bad.sum()))
            x = x * std
        elif leaf == 'ln_gamma':
            x = np.ones(shape)
        else:
            x = np.zeros(shape)
        parts.append(np.asarray(x, dtype=np.float32).ravel())
    return np.concatenate(parts)


class Seq2SeqTransformer(object):
    """``keras_transformer.get_model(...)`` as the checker calls it, on the device.  ``predict([enc, dec])`` -> float32 [N, L, V];
    ``beam(...)`` is the device beam search ``rl4rs.mdpchecker.decoder.beam_search`` runs.  ``max_rows`` bounds the rows of one
    device call (None: chosen per call, at most ``ROW_BUDGET`` floats of probabilities); more users are decoded in chunks."""
    ROW_BUDGET = 1 << 26

    def __init__(self, token_num, embed_dim=256, encoder_num=1, decoder_num=1, head_num=1, hidden_dim=128, dropout_rate=0.05,
                 use_same_embed=False, seed=0, max_rows=None):
        if encoder_num != 1 or decoder_num != 1 or head_num != 1:
            raise ValueError('Seq2SeqTransformer runs encoder_num = decoder_num = head_num = 1 (got %r, %r, %r)'
                             % (encoder_num, decoder_num, head_num))
        if use_same_embed:
            raise ValueError('Seq2SeqTransformer runs use_same_embed=False only')
        if not 0.0 <= dropout_rate < 1.0:
            raise ValueError('dropout_rate %r outside [0, 1)' % (dropout_rate,))
        self.token_num, self.embed_dim, self.hidden_dim = int(token_num), int(embed_dim), int(hidden_dim)
        self.dropout_rate = float(dropout_rate)
        if self.token_num < 4 or self.embed_dim < 2 or self.embed_dim % 2 or self.hidden_dim < 1:
            raise ValueError('token_num >= 4, an even embed_dim and hidden_dim >= 1 are required')
        self.max_rows = None if max_rows is None else int(max_rows)
        self.params = init_params(self.token_num, self.embed_dim, self.hidden_dim, seed)
        self.seed = int(seed)
        self._net = None
        self._adam = None                        # (m, v, steps taken) once fit has run or a file brought them
        self._epochs = 0

    # ---- weights
    def get_weights(self):
        out, o = {}, 0
        for name, shape in param_layout(self.token_num, self.embed_dim, self.hidden_dim):
            n = int(np.prod(shape))
            out[name] = self.params[o:o + n].reshape(shape).copy()
            o += n
        return out

    def set_weights(self, weights):
        """a flat float32 vector in the header's layout, or a dict name -> array as ``get_weights`` returns"""
        if isinstance(weights, dict):
            weights = np.concatenate([np.asarray(weights[name], dtype=np.float32).reshape(shape).ravel()
                                      for name, shape in param_layout(self.token_num, self.embed_dim, self.hidden_dim)])
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.shape != self.params.shape:
            raise ValueError('expected %d parameters, got %r' % (self.params.size, weights.shape))
        self.params = weights.copy()
        if self._net is not None:
            self._net.set_params(self.params)

    def _push_adam(self, net):
        if self._adam is not None:
            m, v, _ = net.adam_state()
            m.copy_(torch.from_numpy(self._adam[0]))
            v.copy_(torch.from_numpy(self._adam[1]))
            net.set_adam_step(self._adam[2])

    def save_weights(self, path):
        """``.npz``: the named weights and, once there is one, the Adam state (moments, steps taken)"""
        extra = {} if self._adam is None else dict(__adam_m=self._adam[0], __adam_v=self._adam[1], __adam_t=self._adam[2])
        np.savez(path, __token_num=self.token_num, __embed_dim=self.embed_dim, __hidden_dim=self.hidden_dim, **extra, **self.get_weights())

    def load_weights(self, path):
        with np.load(path) as z:
            dims = tuple(int(z[k]) for k in ('__token_num', '__embed_dim', '__hidden_dim'))
            if dims != (self.token_num, self.embed_dim, self.hidden_dim):
                raise ValueError('%s holds a model of (token_num, embed_dim, hidden_dim) = %r, this one is %r'
                                 % (path, dims, (self.token_num, self.embed_dim, self.hidden_dim)))
            self.set_weights({k: z[k] for k in z.files if not k.startswith('__')})
            self._adam = (z['__adam_m'].astype(np.float32), z['__adam_v'].astype(np.float32), int(z['__adam_t'])) if '__adam_t' in z.files else None
            if self._net is not None and self._adam is not None:
                self._push_adam(self._net)

    # ---- device
    def _handle(self, src_len, tgt_len, rows):
        """the device handle, rebuilt when a call needs another source length, more positions or more rows"""
        n = self._net
        if n is None or n.src_len != src_len or n.tgt_len < tgt_len or n.max_rows < rows:
            if n is not None:
                n.close()
            self._net = D.DeviceSeq2Seq(self.token_num, self.embed_dim, self.hidden_dim, src_len, max(tgt_len, n.tgt_len if n else 0),
                                        max(rows, n.max_rows if n is not None and n.src_len == src_len else 0), self.params)
            self._push_adam(self._net)
        return self._net

    def reserve(self, src_len, tgt_len, rows):
        """build the device handle once for the largest call to come (it is rebuilt whenever a call needs more than it has)"""
        self._handle(int(src_len), int(tgt_len), int(rows))

    def fit(self, x, y, epochs=20, batch_size=256, shuffle=True, verbose=0):
        """keras' ``model.fit(x=[enc, dec_in], y=dec_out)`` under ``compile('adam', 'sparse_categorical_crossentropy')``: per batch
        one ``rl4rs_seq2seq_loss_grad`` (dropout masks of (seed, number of batches taken so far)) and one Adam step (lr 1e-3, 0.9,
        0.999, eps 1e-7).  ``y`` may carry keras' trailing singleton axis.  Epoch e of a model's life shuffles with
        ``RandomState(seed * 1000003 + e)``.  -> the per-epoch losses (sample-weighted means of the batch losses)."""
        enc, dec_in = (np.ascontiguousarray(a, dtype=np.int32) for a in x)
        y = np.asarray(y)
        if y.ndim == 3:
            y = y[:, :, 0]
        y = np.ascontiguousarray(y, dtype=np.int32)
        if enc.ndim != 2 or dec_in.shape != y.shape or enc.shape[0] != y.shape[0] or not len(enc):
            raise ValueError('fit(x=[encoder tokens [N, S], decoder inputs [N, L]], y=decoder outputs [N, L] or [N, L, 1])')
        N, S, L = enc.shape[0], enc.shape[1], y.shape[1]
        B = min(int(batch_size), N)
        net = self._handle(S, L, B * max(S, L))
        t = net.adam_state()[2]
        history = []
        for _ in range(int(epochs)):
            order = np.random.RandomState(self.seed * 1000003 + self._epochs).permutation(N) if shuffle else np.arange(N)
            losses, sizes = [], []
            for a in range(0, N, B):
                idx = order[a:a + B]
                losses.append(net.loss_grad(enc[idx], dec_in[idx], y[idx], self.dropout_rate, self.seed, t))
                net.adam_step()
                t += 1
                sizes.append(len(idx))
            self._epochs += 1
            history.append(float(np.average(torch.cat(losses).cpu().numpy().astype(np.float64), weights=sizes)))
            if verbose:
                print('epoch %d - loss: %.4f' % (self._epochs, history[-1]))
        self.params = net.params().cpu().numpy().copy()
        m, v, t = net.adam_state()
        self._adam = (m.cpu().numpy().copy(), v.cpu().numpy().copy(), t)
        return history

    def _rows_per_call(self, per_user):
        """(users per call, max_rows) for calls that need ``per_user`` activation rows per user"""
        widest = max(self.token_num + 3, 2 * self.embed_dim, self.hidden_dim)
        cap = max(per_user, min(self.ROW_BUDGET // widest, ((1 << 31) - 1) // (4 * widest)))
        if self.max_rows is not None:
            if self.max_rows < per_user:
                raise ValueError('max_rows %d is below the %d rows one user needs' % (self.max_rows, per_user))
            cap = self.max_rows
        return cap // per_user, cap

    def predict(self, x):
        enc, dec = (np.asarray(a) for a in x)
        if enc.ndim != 2 or dec.ndim != 2 or enc.shape[0] != dec.shape[0]:
            raise ValueError('predict([encoder tokens [N, S], decoder tokens [N, L]])')
        N, S, L = enc.shape[0], enc.shape[1], dec.shape[1]
        users, rows = self._rows_per_call(max(S, L))
        net = self._handle(S, L, min(rows, N * max(S, L)))
        out = np.empty((N, L, self.token_num), dtype=np.float32)
        for a in range(0, N, users):
            out[a:a + users] = net.forward(enc[a:a + users], dec[a:a + users]).cpu().numpy()
        return out

    def first_step_probs(self, enc):
        """float32 device tensor [N, V]: the distribution of the first target token"""
        enc = np.asarray(enc)
        N, S = enc.shape
        users, rows = self._rows_per_call(S)
        net = self._handle(S, 1, min(rows, N * S))
        start = np.full((N, 1), START, dtype=np.int32)
        return torch.cat([net.forward(enc[a:a + users], start[a:a + users])[:, 0] for a in range(0, N, users)])

    def beam(self, enc, beam_size, target_len, candidates=None, want_step_probs=False):
        """-> (paths int64 [N, K, target_len + 1], scores float64 [N, K], step_probs float32 [N, K, target_len] or None), numpy.
        ``candidates``: int [N, C] token ids per user; tokens outside count as probability 0 from the second step on."""
        enc = np.asarray(enc)
        N, S = enc.shape
        K, T = int(beam_size), int(target_len)
        bits = None
        if candidates is not None:
            cand = torch.as_tensor(np.asarray(candidates), dtype=torch.int64)
            if cand.shape[1] < K:
                raise ValueError('candidates_size %d is below beam_size %d' % (cand.shape[1], K))
            onehot = torch.zeros((N, (self.token_num + 31) // 32 * 32), dtype=torch.int64)
            onehot.scatter_(1, cand, 1)
            w = onehot.reshape(N, -1, 32) << torch.arange(32, dtype=torch.int64)
            bits = w.sum(-1).numpy().astype(np.uint32)
        users, rows = self._rows_per_call(max(K, S, 1))
        net = self._handle(S, T + 1, min(rows, N * max(K, S, 1)))
        paths, scores, sps = [], [], []
        for a in range(0, N, users):
            p, s, sp = net.beam(enc[a:a + users], K, T, None if bits is None else bits[a:a + users], want_step_probs)
            paths.append(p.cpu().numpy().astype(np.int64))
            scores.append(s.cpu().numpy())
            if want_step_probs:
                sps.append(sp.cpu().numpy())
        return np.concatenate(paths), np.concatenate(scores), (np.concatenate(sps) if want_step_probs else None)


# ---------------------------------------------------------------- rl4rs/mdpchecker/decoder.py
def _device_model(model):
    if not isinstance(model, Seq2SeqTransformer):
        raise TypeError('the device decoder runs a rl4rs_amd.mdpchecker.Seq2SeqTransformer, not %s (there is no CPU path)'
                        % type(model).__name__)
    return model


def token_probs(model, batch_inputs, batch_outputs):
    """probabilities [N, V] of the token that follows ``batch_outputs``"""
    return _device_model(model).predict([np.array(batch_inputs), np.array(batch_outputs)])[:, -1]


def decode_step(model, batch_inputs, batch_outputs, candidates=None, beam_size=1):
    """[N, beam_size, 2] float64: (probability, token) of the ``beam_size`` likeliest next tokens, best first; ``candidates``
    int [N, C]: tokens outside count as probability 0"""
    predicts = torch.from_numpy(token_probs(model, batch_inputs, batch_outputs))
    if candidates is not None:
        mask = torch.zeros_like(predicts)
        mask.scatter_(1, torch.as_tensor(np.asarray(candidates), dtype=torch.int64), 1.0)
        predicts = predicts * mask
    probs, index = torch.topk(predicts, int(beam_size), dim=1)
    return np.stack([probs.numpy().astype(np.float64), index.numpy().astype(np.float64)], axis=-1)


def beam_search(model, encode_input, beam_size, target_len, use_candidates=False, candidates_size=None):
    """The reference's beam_search: ``output_topk`` int64 [N, beam_size, target_len + 1] (column 0 = <START>) and ``beam_score``
    float64 [N, beam_size], products of probabilities, best beam first.  ``use_candidates``: from the second step on only the
    ``candidates_size`` likeliest first tokens of each user count."""
    paths, scores, _ = beam_search_steps(model, encode_input, beam_size, target_len, use_candidates, candidates_size, False)
    return paths, scores


def beam_search_steps(model, encode_input, beam_size, target_len, use_candidates=False, candidates_size=None, want_step_probs=True):
    """``beam_search`` with the probability of every chosen token along every surviving path as a third result [N, K, target_len]"""
    model = _device_model(model)
    enc = np.asarray(encode_input)
    candidates = None
    if use_candidates:
        if candidates_size is None or int(candidates_size) < int(beam_size):
            raise ValueError('use_candidates needs candidates_size >= beam_size (got %r, beam_size %r)' % (candidates_size, beam_size))
        candidates = torch.topk(model.first_step_probs(enc), int(candidates_size), dim=1).indices.cpu().numpy()
    return model.beam(enc, beam_size, target_len, candidates, want_step_probs)


# ---------------------------------------------------------------- script/mdpchecker: datasets
def source_len_of(name):
    """mdp_checker.py:19-24"""
    if 'recsys15' in name:
        return 8
    if 'cikm2016' in name:
        return 5
    return 16


def rl4rs_sessions(records):
    """preprocess.py's ``rl4rs`` branch: dataset-A records -> ``'sessionid items'`` lines (no header): the last 16 history ids and
    the first 5 exposed items of every record with at least 16 history ids"""
    out = []
    for x in records:
        f = x.split('@')
        sequence_id = [int(v) for v in f[5].split(',')]
        items = [int(v) for v in f[3].split(',')]
        if len(sequence_id) >= 16:
            out.append(f[1] + ' ' + ','.join(str(v) for v in sequence_id[-16:] + items[:5]))
    return out


def build_dataset(lines, name, target_len=5):
    """mdp_checker.py:19-84 on ``'sessionid items'`` lines (header and trailing empty line already dropped): windows, one token
    dictionary grown over the sources and then the targets, <START> / <END> / <PAD> framing.  The window strides of the files other
    than rl4rs and cikm2016 draw from ``np.random.seed(1)`` as the script does (the global generator is reseeded here)."""
    source_len = source_len_of(name)
    fixed = 'rl4rs' in name or 'cikm2016' in name
    np.random.seed(1)
    source_tokens, target_tokens = [], []
    for sample in lines:
        _, items = sample.split(' ')
        item_list = items.split(',')
        if len(item_list) < source_len + target_len:
            continue
        if fixed:
            source_tokens.append(item_list[:source_len])
            target_tokens.append(item_list[source_len:source_len + target_len])
            continue
        i = 0
        while i + source_len + target_len < len(item_list):
            source_tokens.append(item_list[i:i + source_len])
            target_tokens.append(item_list[i + source_len:i + source_len + target_len])
            i = i + np.random.randint(source_len, source_len + target_len) // 6
    token_dict = {'<PAD>': PAD, '<START>': START, '<END>': END}
    for token_list in (source_tokens, target_tokens):
        for tokens in token_list:
            for token in tokens:
                if token not in token_dict:
                    token_dict[token] = len(token_dict)
    enc = [['<START>'] + t + ['<END>'] for t in source_tokens]
    dec = [['<START>'] + t + ['<END>'] for t in target_tokens]
    out = [t + ['<END>', '<PAD>'] for t in target_tokens]

    def ids(rows):
        width = max(len(r) for r in rows) if rows else 0
        return np.array([[token_dict[t] for t in r + ['<PAD>'] * (width - len(r))] for r in rows], dtype=np.int32).reshape(len(rows), width)
    return dict(encode_input=ids(enc), decode_input=ids(dec), decode_output=ids(out)[:, :, None], token_dict=token_dict,
                token_num=len(token_dict), source_len=source_len, target_len=target_len)


# ---------------------------------------------------------------- script/mdpchecker: the two experiments
def _ranks(x):
    """average-tie ranks (scipy.stats.rankdata's default)"""
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind='stable')
    xs = x[order]
    first = np.concatenate(([True], xs[1:] != xs[:-1]))
    start = np.flatnonzero(first)
    end = np.concatenate((start[1:], [x.size]))
    avg = (start + end - 1) / 2.0 + 1.0
    ranks = np.empty(x.size)
    ranks[order] = np.repeat(avg, end - start)
    return ranks


def spearman(x, y):
    """Spearman's rho: Pearson of the average-tie ranks (nan for a constant input, as scipy's)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.corrcoef(_ranks(x), _ranks(y))[0][1]


def experiment_II(beam_size, greedy_score, beam_score, beam_score_hot):
    """mdp_checker.py:149-167 -> (top-20 %, greedy, hot top-5 %, hot top-20 %) mean score ratios against the top-5 % beams.  The
    5 % / 20 % slices are ``int(beam_size * 0.05)`` / ``int(beam_size * 0.2)`` of ``beam_size`` for the hot beams too, as written."""
    n5, n20 = int(beam_size * 0.05), int(beam_size * 0.2)
    with np.errstate(divide='ignore', invalid='ignore'):
        top5 = np.nanmean(beam_score[:, :n5], axis=1)
        return tuple(float(np.nanmean(np.nanmean(s, axis=1) / top5))
                     for s in (beam_score[:, :n20], greedy_score, beam_score_hot[:, :n5], beam_score_hot[:, :n20]))


def experiment_I(step_probs):
    """mdp_checker.py:169-191 from the per-step probabilities [N, K, T] of the K beams: Pearson and Spearman correlation of every
    prefix score with the sequence score, nan -> 1, mean over users -> [T, 2]"""
    probs = np.asarray(step_probs, dtype=np.float64)
    N, _, T = probs.shape
    metrics = np.zeros((N, T, 2))
    for n in range(N):
        seq = np.multiply.reduce(probs[n], axis=1)
        for i in range(T):
            pre = np.multiply.reduce(probs[n][:, :i + 1], axis=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                metrics[n, i] = (np.corrcoef(pre, seq)[0][1], spearman(pre, seq))
    return np.nanmean(np.nan_to_num(metrics, nan=1.0), axis=0)


def check(model, encode_input, name='rl4rs', batch_size=2048, beam_size=100, target_len=5, holdout=10000, verbose=True):
    """mdp_checker.py:133-191 for a trained model: ``random.seed(1)`` sample of ``batch_size`` of the last ``holdout`` sources,
    greedy / beam / hot beam search, both experiments.  Experiment I reads the beam search's own step probabilities where the
    script runs ``beam_size * target_len`` more predictions."""
    hot_beam_size = 20 if 'rl4rs' in name else beam_size
    candidates_size = 6000 if 'cikm2016' in name else hot_beam_size
    random.seed(1)
    pool = [list(r) for r in np.asarray(encode_input)[-holdout:]]
    enc = np.array(random.sample(pool, min(batch_size, len(pool))))
    per_user = max(beam_size, hot_beam_size, enc.shape[1])       # one handle for the three searches and the first-step probabilities
    model.reserve(enc.shape[1], target_len + 1, min(model._rows_per_call(per_user)[1], len(enc) * per_user))
    _, greedy_score = beam_search(model, enc, 1, target_len)
    _, beam_score, step_probs = beam_search_steps(model, enc, beam_size, target_len)
    _, hot_score = beam_search(model, enc, hot_beam_size, target_len, use_candidates=True, candidates_size=candidates_size)
    two = experiment_II(beam_size, greedy_score, beam_score, hot_score)
    one = experiment_I(step_probs)
    if verbose:
        print('experiment II results')
        print('top_5_percent_score top_20_percent_score greedy_score hot_5_percent_score hot_20_percent_score')
        print(1, *two)
        print('experiment I results')
        print('corrcoef', ' ', 'spearman')
        print(one)
    return dict(experiment_II=two, experiment_I=one)


def run(name, dataset_dir, epochs=20, batch_size=256, holdout=10000, check_batch_size=2048, beam_size=100, seed=0, weights_file=None,
        verbose=True):
    """script/mdpchecker/mdp_checker.py end to end: ``dataset_dir/name.csv`` (a header line, then ``sessionid items`` lines; the
    script's ``split('\\n')[1:-1]`` is kept, so the LAST line is dropped too: the reference's preprocessing writes no trailing newline
    and loses its last session there.  From dataset-A records: ``'\\n'.join(['sessionid items'] + rl4rs_sessions(records))`` is that
    file, byte for byte) ->
    windows and dictionaries, the model at the script's sizes, ``fit`` on all but the last ``holdout`` samples, weights saved to
    ``weights_file`` (default ``name.npz`` in the working directory) and loaded back, both experiments on a ``random.seed(1)``
    sample of the hold-out.  -> dict(history, experiment_II, experiment_I, token_num, samples)"""
    import os
    lines = open(os.path.join(dataset_dir, name + '.csv')).read().split('\n')[1:-1]
    data = build_dataset(lines, name)
    if verbose:
        print('sample lens:', len(data['encode_input']))
        print('token_dict lens:', data['token_num'])
    model = Seq2SeqTransformer(token_num=data['token_num'], embed_dim=256, encoder_num=1, decoder_num=1, head_num=1, hidden_dim=128,
                               dropout_rate=0.05, use_same_embed=False, seed=seed)
    history = model.fit(x=[data['encode_input'][:-holdout], data['decode_input'][:-holdout]], y=data['decode_output'][:-holdout],
                        epochs=epochs, batch_size=batch_size, shuffle=True, verbose=2 if verbose else 0)
    weights_file = weights_file or name + '.npz'
    model.save_weights(weights_file)
    model.load_weights(weights_file)
    out = check(model, data['encode_input'], name=name, batch_size=check_batch_size, beam_size=beam_size,
                target_len=data['target_len'], holdout=holdout, verbose=verbose)
    out.update(history=history, token_num=data['token_num'], samples=len(data['encode_input']))
    return out

