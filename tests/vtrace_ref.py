"""float64 restatement of V-trace (include/rl4rs_hip.h, "V-trace") and of the V-trace loss on the mask policy.

PARITY UNPINNED: the arithmetic follows RLlib 1.5.1's ``vtrace_tf.from_importance_weights`` and ``VTraceLoss`` (ray is not
vendored).  The policy forward and the autograd of the A2C-form loss are ``oracle.policy``'s."""
import numpy as np

from oracle import policy as OP


def vtrace(behaviour_logp, target_logp, values, rewards, bootstrap_value=None, dones=None, gamma=1.0, clip_rho=1.0, clip_pg_rho=1.0):
    """Time-major [T, B] arrays -> dict(vs, pg_adv, rho), all float64.  gamma and the two thresholds are float32 at the C ABI:
    they are rounded to float32 first, everything else is float64 arithmetic on the inputs as given."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    blp, tlp, V, r = f(behaviour_logp), f(target_logp), f(values), f(rewards)
    T, B = V.shape
    gamma, clip_rho, clip_pg_rho = float(np.float32(gamma)), float(np.float32(clip_rho)), float(np.float32(clip_pg_rho))
    boot = np.zeros(B) if bootstrap_value is None else f(bootstrap_value)
    done = np.zeros((T, B)) if dones is None else (np.asarray(dones) != 0).astype(np.float64)
    rho = np.exp(tlp - blp)
    disc = gamma * (1.0 - done)
    c = np.minimum(1.0, rho)
    vs, pg = np.zeros((T, B)), np.zeros((T, B))
    acc = np.zeros(B)
    v_next, vs_next = boot, boot
    for t in range(T - 1, -1, -1):
        delta = np.minimum(clip_rho, rho[t]) * (r[t] + disc[t] * v_next - V[t])
        acc = delta + disc[t] * c[t] * acc
        vs[t] = V[t] + acc
        pg[t] = np.minimum(clip_pg_rho, rho[t]) * (r[t] + disc[t] * vs_next - V[t])
        v_next, vs_next = V[t], vs[t]
    return dict(vs=vs, pg_adv=pg, rho=rho)


def vtrace_stats(behaviour_logp, target_logp, vs, pg_adv, clip_rho=1.0):
    """{sum rho, sum min(rho, clip_rho), sum vs, sum pg_adv} in float64 of the arrays as given (the device's float32 outputs)."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    rho = np.exp(f(target_logp) - f(behaviour_logp))
    return np.array([rho.sum(), np.minimum(rho, float(np.float32(clip_rho))).sum(), f(vs).sum(), f(pg_adv).sum()])


def kept_rows(R, T, B, drop_last):
    """Row indices (of the [R, T, B] order) the loss runs over: every step, or all but each rollout's last."""
    Te = T - 1 if drop_last else T
    return np.concatenate([np.arange(r * T * B, r * T * B + Te * B) for r in range(R)])


def vtrace_rollouts(R, T, B, behaviour_logp, target_logp, values, rewards, dones=None, gamma=1.0, clip_rho=1.0, clip_pg_rho=1.0,
                    drop_last=True):
    """V-trace per rollout of flat [R * T * B] arrays -> (vs, pg_adv) float64 [R * T * B], zeros on dropped rows.  drop_last: steps
    0 .. T-2 with values[T-1] as the bootstrap; else all T steps and a zero bootstrap."""
    sh = lambda x: None if x is None else np.asarray(x).reshape(R, T, B)
    blp, tlp, V, r, dn = sh(behaviour_logp), sh(target_logp), sh(values), sh(rewards), sh(dones)
    Te = T - 1 if drop_last else T
    vs, pg = np.zeros((R, T, B)), np.zeros((R, T, B))
    for k in range(R):
        o = vtrace(blp[k, :Te], tlp[k, :Te], V[k, :Te], r[k, :Te], V[k, T - 1] if drop_last else None, None if dn is None else dn[k, :Te],
                   gamma, clip_rho, clip_pg_rho)
        vs[k, :Te], pg[k, :Te] = o['vs'], o['pg_adv']
    return vs.reshape(-1), pg.reshape(-1)


def vtrace_loss_and_grad(flat, obs, mask, actions, vs, pg_adv, rows, vf_coeff=0.5, ent_coeff=0.01, od=256, hid=64, A=284):
    """-sum(logp * pg_adv) + vf_coeff * 0.5 * sum((V - vs)^2) - ent_coeff * sum(H) over ``rows`` with vs / pg_adv held constant
    -> (grad flat float64, stats[4] sums)."""
    rows = np.asarray(rows)
    return OP.loss_and_grad(0, flat, np.asarray(obs)[rows], None if mask is None else np.asarray(mask)[rows], np.asarray(actions)[rows],
                            np.asarray(pg_adv)[rows], np.asarray(vs)[rows], vf_coeff=vf_coeff, ent_coeff=ent_coeff, od=od, hid=hid, A=A)
