"""float64 restatement of the on-device DQN (include/rl4rs_hip.h, "On-device DQN"): replay ring arithmetic, proportional
prioritized sampling, the (double-)Q Huber loss with its hand-written gradient, the per-variable-clipped Adam step.

Test infrastructure only.  PARITY UNPINNED: ray 1.5.1 (dqn_tf_policy, PrioritizedReplayBuffer, minimize_and_clip) is absent, so this
restates their published form as script/modelfree_train.py:106-133 configures them; tests/test_dqn_host.py checks the gradient
below against torch float64 autograd of the same loss."""
import numpy as np

from oracle import policy as OP

F32_MIN = OP.F32_MIN


# ---- replay ring -----------------------------------------------------------------------------------------------------
def capacity_rollouts(buffer_size, T, B):
    """Whole rollouts the ring holds: the one deviation from RLlib's per-timestep ring."""
    return max(1, int(buffer_size) // (int(T) * int(B)))


def slot_of_push(push_index, buffer_size, T, B):
    """Rollout slot that push number ``push_index`` (0-based) lands in; the oldest rollout is evicted whole."""
    return push_index % capacity_rollouts(buffer_size, T, B)


def filled_rows(pushes, buffer_size, T, B):
    return min(pushes, capacity_rollouts(buffer_size, T, B)) * T * B


def row_fields(idx, T, B):
    """(slot, t, b, done, successor row or -1) of ring row ``idx`` in the order (slot * T + t) * B + b."""
    idx = np.asarray(idx, dtype=np.int64)
    slot, r = idx // (T * B), idx % (T * B)
    t, b = r // B, r % B
    done = t == T - 1
    return slot, t, b, done, np.where(done, -1, idx + B)


# ---- sampling --------------------------------------------------------------------------------------------------------
def uniform_select(u, n):
    return np.minimum(np.floor(np.asarray(u, dtype=np.float64) * n).astype(np.int64), n - 1)


def prioritized_select(prio, u):
    """idx = smallest i whose inclusive float64 prefix sum exceeds u * total -> (idx, distance of the draw's mass to the nearest
    prefix boundary, total)."""
    c = np.cumsum(np.asarray(prio, dtype=np.float64))
    total = c[-1]
    mass = np.asarray(u, dtype=np.float64) * total
    idx = np.minimum(np.searchsorted(c, mass, side='right'), len(c) - 1)
    edges = np.concatenate([[0.0], c])
    dist = np.minimum(np.abs(mass - edges[idx]), np.abs(edges[idx + 1] - mass))
    return idx, dist, total


def is_weights(prio, idx, beta):
    """RLlib PrioritizedReplayBuffer.sample: (n p_i / total)^-beta / (n p_min / total)^-beta."""
    p = np.asarray(prio, dtype=np.float64)
    n, total = len(p), p.sum()
    return (n * p[idx] / total) ** -beta / (n * p.min() / total) ** -beta


def update_priorities(prio, max_priority, idx, td, alpha, eps=1e-6):
    """Sequential RLlib update: a later batch position overwrites an earlier one -> (priorities, max_priority)."""
    prio = np.array(prio, dtype=np.float64)
    for i, t in zip(np.asarray(idx), np.asarray(td, dtype=np.float64)):
        pr = abs(t) + eps
        prio[i] = pr ** alpha
        max_priority = max(max_priority, pr)
    return prio, max_priority


# ---- loss ------------------------------------------------------------------------------------------------------------
def unpack_bits(bits, A):
    b = np.ascontiguousarray(bits).view(np.uint32)
    return ((b[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(b.shape[0], -1)[:, :A].astype(np.float64)


def next_action(flat, tflat, next_obs, next_mask, done, double_q, od, hid, A):
    """-> (a* [N] first maximum of the masked Q(s') of the selecting net, boot [N] = non-terminal and some action allowed,
    gap [N] = top-two gap of that masked row (inf for rows that do not bootstrap)).  Terminal rows' successors are not read."""
    N = len(done)
    done = np.asarray(done).astype(bool)
    nobs = np.where(done[:, None], 0.0, np.asarray(next_obs, dtype=np.float64))
    mask = np.ones((N, A)) if next_mask is None else np.asarray(next_mask, dtype=np.float64)
    q_sel = OP.forward(flat if double_q else tflat, nobs, mask, od, hid, A)[0]
    astar = q_sel.argmax(axis=1)
    boot = ~done & (mask > 0).any(axis=1)
    top = np.sort(q_sel, axis=1)[:, -2:]
    gap = np.where(boot, top[:, 1] - top[:, 0], np.inf)
    return astar, boot, gap


def dqn_loss_and_grad(flat, tflat, obs, act, rew, done, next_obs, next_mask, weights=None, gamma=1.0, double_q=True,
                      od=256, hid=64, A=284, astar=None):
    """-> dict(loss, grad, td, y, qsa, astar, boot, gap, stats).  ``astar`` (optional) overrides the argmax on the rows that
    bootstrap (teacher-forcing with the device's choice on near-ties).  A non-terminal row whose successor allows no action gets
    y = r like a terminal row (the header's rule).  loss = mean(w * huber(Q(s)[a] - y))."""
    flat = np.asarray(flat, dtype=np.float64)
    tflat = np.asarray(tflat, dtype=np.float64)
    N = len(act)
    act = np.asarray(act, dtype=np.int64)
    done_b = np.asarray(done).astype(bool)
    a_ref, boot, gap = next_action(flat, tflat, next_obs, next_mask, done_b, double_q, od, hid, A)
    a_use = a_ref if astar is None else np.where(boot, np.asarray(astar, dtype=np.int64), a_ref)
    nobs = np.where(done_b[:, None], 0.0, np.asarray(next_obs, dtype=np.float64))
    q_t = OP.forward(tflat, nobs, None, od, hid, A)[0]
    qt = np.where(boot, q_t[np.arange(N), a_use], 0.0)
    rew = np.asarray(rew, dtype=np.float64)
    y = np.where(boot, rew + gamma * qt, rew)
    W1, b1, W2, b2 = OP._split(flat, od, hid, A)
    x = np.asarray(obs, dtype=np.float64)
    h = np.tanh(x @ W1 + b1)
    qsa = (h * W2[:, act].T).sum(axis=1) + b2[act]
    td = qsa - y
    ad = np.abs(td)
    hub = np.where(ad < 1.0, 0.5 * td * td, ad - 0.5)
    w = np.ones(N) if weights is None else np.asarray(weights, dtype=np.float64)
    g = w * np.clip(td, -1.0, 1.0) / N
    gW2 = np.zeros_like(W2)
    gb2 = np.zeros_like(b2)
    np.add.at(gW2.T, act, g[:, None] * h)
    np.add.at(gb2, act, g)
    dpre = g[:, None] * W2[:, act].T * (1.0 - h * h)
    grad = np.concatenate([(x.T @ dpre).ravel(), dpre.sum(axis=0), gW2.ravel(), gb2])
    stats = np.array([(w * hub).sum(), qsa.sum(), y.sum(), ad.sum()])
    return dict(loss=(w * hub).mean(), grad=grad, td=td, y=y, qsa=qsa, astar=a_use, astar_ref=a_ref, boot=boot, gap=gap, stats=stats)


def dqn_loss_autograd(flat, y, obs, act, weights=None, od=256, hid=64, A=284):
    """torch float64 autograd of mean(w * huber(Q(s)[a] - y)) with the targets held constant -> (loss, grad)."""
    import torch
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)
    p = t(flat).clone().requires_grad_(True)
    ae = A + 1
    o = 0
    W1 = p[o:o + od * hid].reshape(od, hid); o += od * hid
    b1 = p[o:o + hid]; o += hid
    W2 = p[o:o + hid * ae].reshape(hid, ae); o += hid * ae
    b2 = p[o:o + ae]
    q = torch.tanh(t(obs) @ W1 + b1) @ W2 + b2
    qsa = q.gather(1, torch.as_tensor(np.asarray(act), dtype=torch.int64)[:, None])[:, 0]
    hub = torch.nn.functional.huber_loss(qsa, t(y), reduction='none', delta=1.0)
    w = torch.ones_like(hub) if weights is None else t(weights)
    loss = (w * hub).mean()
    loss.backward()
    return loss.item(), p.grad.numpy()


def adam_clip_by_var(flat, m, v, t, grad, lr, var_clip, od, hid, A, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.clip_by_norm per variable (W1, b1, W2e, b2e), then oracle.policy.adam_update -> (flat, m, v, t)."""
    g = np.array(grad, dtype=np.float64)
    ends = np.cumsum([od * hid, hid, hid * (A + 1), A + 1])
    lo = 0
    for hi in ends:
        norm = np.sqrt((g[lo:hi] ** 2).sum())
        if var_clip > 0 and norm > var_clip:
            g[lo:hi] *= var_clip / norm
        lo = hi
    return OP.adam_update(flat, m, v, t, g, lr, beta1, beta2, eps)
