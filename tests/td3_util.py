"""TD3 on the engine (csrc/plan_td3.inl, csrc/td3_kernels.h) against a float64 restatement of the update.

Nothing in the reference pins TD3 and oracle/ knows no TD3, so stable-baselines 2.10.1 `td3/td3.py` / `td3/policies.py` are restated
here in torch float64 with autograd, as tests/ppo_util.py restates PPO2: the ReLU policy with its tanh output, the twin critics on
[obs, action], the smoothed target action, the clipped double-Q backup (no gradient through it), the two TF-Adams (epsilon 1e-8)
with step counts of their own and the Polyak average over every `model/` variable.  The order stable-baselines leaves to
TensorFlow is the project's: every gradient and metric at the parameters the update began with, both Adam steps,
then the Polyak average of the stepped parameters.  The same helpers drive a handle of the emulation build
(tests/test_hostemu_td3.py) and of the device (tests/test_gpu_td3.py).

Tolerances are the project's: gathered minibatch tensors bit-exact; forward |d| <= 1e-5 + 1e-4 |ref|; every gradient
tensor within 1e-3 max|g|; parameters after n updates max |d| <= 0.3 lr n and mean |d| <= 0.02 lr n per tensor; metrics as forward.
A row within MARGIN of a branch boundary (|sigma eps| at c, |pi_target + noise| at 1, q1_target = q2_target) could take the other
branch in float32, and a hidden unit within RELU_MARGIN of 0 the other side of its ReLU: `Ref.update` reports the smallest such
distances and every check asserts, on the reference alone and before anything is compared, that none is that close and that both
sides of each branch occur."""
from collections import OrderedDict

import numpy as np
import torch

from grasp_rl import _capi
from grasp_rl.engine import Td3Engine

MARGIN = 1e-5            # loss branches
RELU_MARGIN = 2e-8       # the project's frozen sign-ambiguity bound of a ReLU unit
SIGMA, CLIP = 0.4, 0.5   # sigma eps beyond c for |eps| > 1.25: a tenth of the draws on each side
N_UPDATES = 6
A_MAX = 64               # check_cfg: act_dim <= 64
DELAY_RUNS = [(d, f) for d in (1, 2, 3) for f in (0, 1)]      # (policy_delay, first_step) of the delay tests

# The smallest shapes that cross each edge of the new code.  `seed`: the data seed, searched per case ON THE CPU WITH THE REFERENCE
# ONLY (find_seed below: the first of 0, 1, 2, ... whose six updates keep every margin and show both sides of every branch in every
# update, at each policy_delay 1, 2, 3 and first_step 0, 1 the tests run); `margin`: the smallest loss-branch distance of all of
# those updates at that seed.
CASES = {
    "default": dict(obs_dim=20, A=5, B=64, layers=(64, 64), seed=0, margin=2.1e-04),                   # the shipped widths; obs_dim % 4 == 0: the gather's 16-byte rows
    "odd": dict(obs_dim=13, A=3, B=7, layers=(24, 17, 9), seed=44, margin=8.5e-04),                    # nothing a multiple of a tile or of 4: scalar gather, v1 GEMMs
    "one_layer_A1": dict(obs_dim=11, A=1, B=33, layers=(8,), seed=2, margin=7.1e-05),                  # L = 1 has no middle backward level; A = 1: a half-used pair
    "depth_4": dict(obs_dim=9, A=2, B=16, layers=(8, 7, 6, 5), seed=2, margin=5.7e-04),                # GRL_MAX_LAYERS
    "width_300": dict(obs_dim=30, A=4, B=16, layers=(300, 20), seed=0, margin=8.4e-04),                # a width beyond 256: the act path's launch list + td3_pi
    "two_blocks": dict(obs_dim=6, A=2, B=300, layers=(16, 16), seed=1, margin=2.5e-05),                # two loss blocks, the second with 44 live rows
    "block_256": dict(obs_dim=6, A=2, B=256, layers=(8,), seed=0, margin=8.1e-05),                     # exactly one full block
    "A_max": dict(obs_dim=10, A=A_MAX, B=8, layers=(16,), seed=0, margin=2.4e-04),                     # the largest act_dim the config check admits
    "norm_1": dict(obs_dim=20, A=5, B=32, layers=(16, 16), seed=1, margin=2.3e-05, normalize=1),       # sample-time VecNormalize with non-trivial statistics
    # (added) obs_dim + A a multiple of 4 with obs_dim not: no padding column; plan_td3.inl: ldq = rup(obs_dim + act_dim, 4), vec4 off
    "no_padding": dict(obs_dim=5, A=3, B=9, layers=(12,), seed=13, margin=2.0e-03),
}


def param_names(L):
    out = []
    for scope in ("model", "target"):
        for net, last in (("pi", "dense"), ("values_fn/qf1", "qf1"), ("values_fn/qf2", "qf2")):
            for l in range(L):
                out += ["%s/%s/fc%d/kernel:0" % (scope, net, l), "%s/%s/fc%d/bias:0" % (scope, net, l)]
            out += ["%s/%s/%s/kernel:0" % (scope, net, last), "%s/%s/%s/bias:0" % (scope, net, last)]
    return out


def param_shapes(obs_dim, A, layers):
    sh = OrderedDict()
    for n in param_names(len(layers)):
        pi = "/pi/" in n
        part = n.split("/")[-2]
        if part.startswith("fc"):
            l = int(part[2:])
            k = (obs_dim if pi else obs_dim + A) if l == 0 else layers[l - 1]
            sh[n] = (k, layers[l]) if n.endswith("kernel:0") else (layers[l],)
        else:
            out = A if pi else 1
            sh[n] = (layers[-1], out) if n.endswith("kernel:0") else (out,)
    return sh


def init_params(obs_dim, A, layers, seed, pi_gain=2.5):
    """He-scaled normal kernels, biases away from zero, the target scope drawn on its own (a Polyak average that copied would
    show), and a policy output gain that puts |pi| above 0.9 for a share of the rows."""
    rng = np.random.default_rng(4000 + seed)
    P = OrderedDict()
    for n, shp in param_shapes(obs_dim, A, layers).items():
        if n.endswith("kernel:0"):
            gain = pi_gain if "/pi/dense/" in n else (1.0 if n.split("/")[-2].startswith("qf") else np.sqrt(2.0))
            P[n] = (rng.normal(0.0, 1.0, shp) * gain / np.sqrt(shp[0])).astype(np.float32)
        else:
            P[n] = rng.uniform(-0.3, 0.3, shp).astype(np.float32)
    return P


# ------------------------------------------------------------------------------------------------- float64 restatement
def mlp64(T, scope, last, x, L):
    """(output pre-activation, smallest |hidden pre-activation|)"""
    h, near = x, float("inf")
    for l in range(L):
        z = h @ T["%s/fc%d/kernel:0" % (scope, l)] + T["%s/fc%d/bias:0" % (scope, l)]
        near = min(near, float(z.detach().abs().min()))
        h = torch.relu(z)
    return h @ T["%s/%s/kernel:0" % (scope, last)] + T["%s/%s/bias:0" % (scope, last)], near


class Ref:
    """Parameters, two Adam states with separate step counts, and one `update` per minibatch, all float64."""

    def __init__(self, P, case, lr=3e-4, tau=0.005, gamma=0.99, sigma=SIGMA, clip=CLIP):
        self.L = len(case["layers"])
        self.lr, self.tau, self.gamma, self.sigma, self.clip = lr, tau, gamma, sigma, clip
        self.T = OrderedDict((n, torch.tensor(np.asarray(a, np.float64))) for n, a in P.items())
        self.pi_names = [n for n in self.T if n.startswith("model/pi/")]
        self.qf_names = [n for n in self.T if n.startswith("model/values_fn/")]
        self.m = {n: torch.zeros_like(self.T[n]) for n in self.pi_names + self.qf_names}
        self.v = {n: torch.zeros_like(self.T[n]) for n in self.pi_names + self.qf_names}
        self.t_qf = self.t_pi = 0

    def act(self, obs):
        with torch.no_grad():
            return torch.tanh(mlp64(self.T, "model/pi", "dense", torch.tensor(np.asarray(obs, np.float64)), self.L)[0]).numpy()

    def _adam(self, names, G, t):
        lr_t = self.lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)
        for n in names:
            self.m[n] = self.m[n] + (G[n] - self.m[n]) * (1 - 0.9)
            self.v[n] = self.v[n] + (G[n] ** 2 - self.v[n]) * (1 - 0.999)
            self.T[n] = self.T[n] - lr_t * self.m[n] / (torch.sqrt(self.v[n]) + 1e-8)

    def update(self, mb, eps, update_policy, apply=True):
        """mb: dict of arrays obs, act, rew, next_obs, done (as gathered); eps [B, A].  Returns outputs, gradients, metrics and the
        smallest distances of any row from a branch boundary (`margin`: the loss branches; `relu`: hidden units from 0)."""
        L = self.L
        T = OrderedDict((n, p.clone().requires_grad_(n.startswith("model/"))) for n, p in self.T.items())
        t = {k: torch.tensor(np.asarray(a, np.float64)) for k, a in mb.items()}
        e = torch.tensor(np.asarray(eps, np.float64))
        with torch.no_grad():
            pre_t, r0 = mlp64(T, "target/pi", "dense", t["next_obs"], L)
            raw = self.sigma * e
            noise = torch.clamp(raw, -self.clip, self.clip)
            un = torch.tanh(pre_t) + noise
            a_next = torch.clamp(un, -1.0, 1.0)
            xn = torch.cat([t["next_obs"], a_next], dim=1)
            (q1t, r1), (q2t, r2) = mlp64(T, "target/values_fn/qf1", "qf1", xn, L), mlp64(T, "target/values_fn/qf2", "qf2", xn, L)
            q1t, q2t = q1t[:, 0], q2t[:, 0]
            y = t["rew"] + (1.0 - t["done"]) * self.gamma * torch.minimum(q1t, q2t)
        xs = torch.cat([t["obs"], t["act"]], dim=1)
        (q1, r3), (q2, r4) = mlp64(T, "model/values_fn/qf1", "qf1", xs, L), mlp64(T, "model/values_fn/qf2", "qf2", xs, L)
        q1, q2 = q1[:, 0], q2[:, 0]
        l1, l2 = ((y - q1) ** 2).mean(), ((y - q2) ** 2).mean()
        gq = torch.autograd.grad(l1 + l2, [T[n] for n in self.qf_names])
        G = OrderedDict((n, g.detach()) for n, g in zip(self.qf_names, gq))
        relu = min(r0, r1, r2, r3, r4)
        out = dict(a_next=a_next.numpy(), backup=y.numpy(), q1=q1.detach().numpy(), q2=q2.detach().numpy(), q1t=q1t.numpy(), q2t=q2t.numpy())
        pl = None
        if update_policy:
            pre, r5 = mlp64(T, "model/pi", "dense", t["obs"], L)
            pi = torch.tanh(pre)
            q1pi, r6 = mlp64(T, "model/values_fn/qf1", "qf1", torch.cat([t["obs"], pi], dim=1), L)
            pl = -q1pi[:, 0].mean()
            gp = torch.autograd.grad(pl, [T[n] for n in self.pi_names] + [pi])
            G.update((n, g.detach()) for n, g in zip(self.pi_names, gp))
            out.update(pi=pi.detach().numpy(), q1pi=q1pi[:, 0].detach().numpy(), da=gp[-1].detach().numpy())
            relu = min(relu, r5, r6)
        out["margin"] = min(float((raw.abs() - self.clip).abs().min()), float((un.abs() - 1.0).abs().min()), float((q1t - q2t).abs().min()))
        out["relu"] = relu
        out["sides"] = dict(noise_hi=int((raw > self.clip).sum()), noise_lo=int((raw < -self.clip).sum()), act_hi=int((un > 1.0).sum()),
                            act_lo=int((un < -1.0).sum()), q1_min=int((q1t < q2t).sum()), q2_min=int((q2t < q1t).sum()))
        out["grads"] = OrderedDict((n, g.numpy()) for n, g in G.items())
        out["metrics"] = np.array([float(l1.detach()), float(l2.detach()), float("nan") if pl is None else float(pl.detach()), float(q1.detach().mean()),
                                   float(q2.detach().mean()), 1.0 if update_policy else 0.0])
        if apply:
            self.t_qf += 1
            self._adam(self.qf_names, G, self.t_qf)
            if update_policy:
                self.t_pi += 1
                self._adam(self.pi_names, G, self.t_pi)
                for n in self.pi_names + self.qf_names:
                    tn = "target/" + n[len("model/"):]
                    self.T[tn] = (1.0 - self.tau) * self.T[tn] + self.tau * self.T[n]
        return out


def assert_reference_is_clear(o, what=""):
    """On the reference alone: no row on a branch boundary, no hidden unit on its ReLU's, both sides of every branch taken."""
    assert o["margin"] >= MARGIN, "%s: a row of the reference sits %.2e from a branch boundary: choose another seed" % (what, o["margin"])
    assert o["relu"] >= RELU_MARGIN, "%s: a hidden unit of the reference sits %.2e from 0: choose another seed" % (what, o["relu"])
    assert all(v > 0 for v in o["sides"].values()), "%s: a branch side does not occur: %s" % (what, o["sides"])


# ------------------------------------------------------------------------------------------------- seeded cases
def make_case(name, seed=None, **over):
    """seed None: the seed the table fixes for the case"""
    c = dict(CASES[name])
    c.update(over)
    seed = c["seed"] if seed is None else seed
    c.update(name=name, seed=seed, lr=3e-4, tau=0.005, gamma=0.99)
    od, A, B, layers = c["obs_dim"], c["A"], c["B"], c["layers"]
    rng = np.random.default_rng(9000 + seed)
    c["P"] = init_params(od, A, layers, seed)
    n = c["n_replay"] = max(2 * B, 40)
    norm = c.get("normalize", 0)
    mean, var = (rng.uniform(0.3, 0.8, od), rng.uniform(0.02, 0.11, od)) if norm else (np.zeros(od), np.ones(od))
    c["stats"] = dict(mean=mean, var=var, ret_var=2.3)
    sd = np.sqrt(var)
    c["tr"] = dict(obs=(mean + sd * rng.normal(0.0, 1.0, (n, od))).astype(np.float32), act=rng.uniform(-1.0, 1.0, (n, A)).astype(np.float32),
                   rew=rng.normal(0.0, 1.0, n).astype(np.float32), next_obs=(mean + sd * rng.normal(0.0, 1.0, (n, od))).astype(np.float32),
                   done=(rng.random(n) < 0.2).astype(np.float32))
    c["idx"] = rng.integers(0, n, (N_UPDATES, B)).astype(np.int64)
    c["eps"] = rng.normal(0.0, 1.0, (N_UPDATES, B, A)).astype(np.float32)
    return c


def minibatch(c, u):
    """Update u's rows as the gather leaves them: float32, VecNormalize at sample time in float64 rounded once (normalize = 1)."""
    tr, idx, st = c["tr"], c["idx"][u], c["stats"]
    obs, nxt, rew = tr["obs"][idx], tr["next_obs"][idx], tr["rew"][idx]
    if c.get("normalize", 0) == 1:
        sd = np.sqrt(st["var"] + 1e-8)
        obs = np.clip((obs.astype(np.float64) - st["mean"]) / sd, -10.0, 10.0).astype(np.float32)
        nxt = np.clip((nxt.astype(np.float64) - st["mean"]) / sd, -10.0, 10.0).astype(np.float32)
        rew = np.clip(rew.astype(np.float64) / np.sqrt(st["ret_var"] + 1e-8), -10.0, 10.0).astype(np.float32)
    return dict(obs=obs, act=tr["act"][idx], rew=rew, next_obs=nxt, done=tr["done"][idx])


def is_policy(first_step, u, delay):
    return (first_step + u) % delay == 0


def reference_run(c, n, delay=2, first_step=0):
    ref = Ref(c["P"], c, lr=c["lr"], tau=c["tau"], gamma=c["gamma"])
    outs = [ref.update(minibatch(c, u), c["eps"][u], is_policy(first_step, u, delay)) for u in range(n)]
    return ref, outs


def find_seed(name, tries=200):
    """The search that filled CASES[...]['seed'] / ['margin']: reference only, nothing of the engine."""
    for seed in range(tries):
        c, margin = make_case(name, seed=seed), float("inf")
        try:
            for delay, first_step in DELAY_RUNS:
                for o in reference_run(c, N_UPDATES, delay, first_step)[1]:
                    assert_reference_is_clear(o)
                    margin = min(margin, o["margin"])
        except AssertionError:
            continue
        return seed, margin
    raise RuntimeError("no seed found for " + name)


def engine_config(c, delay=2, seed=None, batch=None, act_batch=4):
    return _capi.make_td3_config(c["obs_dim"], c["A"], layers=c["layers"], batch_size=batch or c["B"], act_batch=act_batch,
                                 replay_capacity=c["n_replay"], normalize=c.get("normalize", 0), gamma=c["gamma"], lr=c["lr"], tau=c["tau"],
                                 policy_delay=delay, target_policy_noise=SIGMA, target_noise_clip=CLIP, seed=c["seed"] if seed is None else seed)


def make_engine(c, backend=None, lib_path=None, delay=2, seed=None):
    cfg, td3 = engine_config(c, delay, seed)
    eng = Td3Engine(cfg, td3, backend=backend, lib_path=lib_path)
    eng.set_parameters(c["P"])
    st = c["stats"]
    eng.set_obs_stats(st["mean"], st["var"], st["ret_var"])
    tr = c["tr"]
    eng.replay_add(tr["obs"], tr["act"], tr["rew"], tr["next_obs"], tr["done"])
    return eng


def close_fwd(x, ref, what):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    assert x.shape == ref.shape, what
    d = np.abs(x - ref)
    assert (d <= 1e-5 + 1e-4 * np.abs(ref)).all(), "%s: max |d| %.3e" % (what, d.max())


def close_grads(G, ref, what=""):
    for n, g in ref.items():
        d = np.abs(np.asarray(G[n], np.float64) - g).max()
        assert d <= 1e-3 * max(np.abs(g).max(), 1e-30), "%s gradient %s: max |d| %.3e against max |g| %.3e" % (what, n, d, np.abs(g).max())


def close_params(P, ref, lr, n_updates):
    for n, t in ref.T.items():
        d = np.abs(np.asarray(P[n], np.float64) - t.numpy())
        assert d.max() <= 0.3 * lr * n_updates + 1e-7, "param %s: max |d| %.3e (lr %.1e, %d updates)" % (n, d.max(), lr, n_updates)
        assert d.mean() <= 0.02 * lr * n_updates + 1e-9, "param %s: mean |d| %.3e" % (n, d.mean())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def state_of(eng):
    """Everything an update moves: parameters, both Adams' moments and beta powers."""
    s = dict(eng.get_parameters())
    for n in ("adam_m", "adam_v", "td3_beta_c", "td3_beta_pi"):
        s[n] = eng.fetch(n)
    return s


def same_state(a, b):
    return [n for n in a if not same_bits(a[n], b[n])]


# ------------------------------------------------------------------------------------------------- the checks both builds run
def fetch_forward(eng, c):
    B, A, F = c["B"], c["A"], c["obs_dim"]
    q = eng.fetch("td3_q", (5, B))
    return dict(xs=eng.fetch("td3_xs", (B, eng.ldq)), xn=eng.fetch("td3_xn", (B, eng.ldq)), rew=eng.fetch("rew", (B,)), done=eng.fetch("done", (B,)),
                a_next=eng.fetch("td3_a_next", (B, A)), noise=eng.fetch("td3_noise", (B, A)), backup=eng.fetch("td3_backup", (B,)),
                q1=q[0], q2=q[1], q1t=q[2], q2t=q[3], q1pi=q[4], pi=eng.fetch("td3_pi", (B, A)), da=eng.fetch("td3_da", (B, A)))


def check_forward(eng, c):
    """One policy update with the caller's idx / eps: the gathered rows bit for bit, then a', the backup, the five critic outputs,
    pi and d a against the reference.  Returns what was fetched (the emulation test compares a second run's bits)."""
    _, (o,) = reference_run(c, 1)
    assert_reference_is_clear(o, c["name"])
    eng.train(1, c["idx"][:1], c["eps"][:1], first_step=0)
    f = fetch_forward(eng, c)
    mb, F, A = minibatch(c, 0), c["obs_dim"], c["A"]
    assert same_bits(f["xs"][:, :F], mb["obs"]) and same_bits(f["xs"][:, F:F + A], mb["act"]) and not f["xs"][:, F + A:].any()
    assert same_bits(f["xn"][:, :F], mb["next_obs"]) and same_bits(f["xn"][:, F:F + A], f["a_next"]) and not f["xn"][:, F + A:].any()
    assert same_bits(f["rew"], mb["rew"]) and same_bits(f["done"], mb["done"]) and same_bits(f["noise"], c["eps"][0])
    for k in ("a_next", "backup", "q1", "q2", "q1t", "q2t", "q1pi", "pi"):
        close_fwd(f[k], o[k], k)
    d = np.abs(f["da"].astype(np.float64) - o["da"]).max()
    assert d <= 1e-3 * np.abs(o["da"]).max(), "d a: max |d| %.3e" % d
    m = eng.metrics()
    assert m.shape == (1, 6)
    close_fwd(m[0], o["metrics"], "metrics")
    return f


def check_gradients(eng, c):
    """Update 0 (policy) and update 1 (critic-only) at policy_delay 2: the bucket after each.  A critic-only update leaves the
    policy's slots as the last policy update summed them (its reduction has no descriptor for them, its Adam no launch over them)."""
    ref, outs = reference_run(c, 2)
    for o in outs:
        assert_reference_is_clear(o, c["name"])
    eng.train(1, c["idx"][:1], c["eps"][:1], first_step=0)
    g0 = eng.get_gradients()
    close_grads(g0, outs[0]["grads"], "policy update")
    assert set(outs[0]["grads"]) == set(g0)
    eng.train(1, c["idx"][1:2], c["eps"][1:2], first_step=1)
    g1 = eng.get_gradients()
    close_grads(g1, outs[1]["grads"], "critic-only update")
    assert not any(n.startswith("model/pi/") for n in outs[1]["grads"])
    for n in g0:
        if n.startswith("model/pi/"):
            assert same_bits(g0[n], g1[n]), n
    close_params(eng.get_parameters(), ref, c["lr"], 2)


def check_delay(make, c, delay, first_step):
    """Six updates, one call each: flags, what a critic-only update must not touch, Adam step counts, parameters."""
    ref, outs = reference_run(c, N_UPDATES, delay, first_step)
    for o in outs:
        assert_reference_is_clear(o, c["name"])
    eng = make(c, delay)
    for u in range(N_UPDATES):
        before = eng.get_parameters()
        eng.train(1, c["idx"][u:u + 1], c["eps"][u:u + 1], first_step=first_step + u)
        after = eng.get_parameters()
        pol = is_policy(first_step, u, delay)
        m = eng.metrics()
        assert m.shape == (1, 6) and m[0, 5] == (1.0 if pol else 0.0)
        frozen = [n for n in before if n.startswith("target/") or n.startswith("model/pi/")]
        changed = [n for n in frozen if not same_bits(before[n], after[n])]
        assert (len(changed) == len(frozen)) if pol else not changed, (u, pol, changed)
        assert all(not same_bits(before[n], after[n]) for n in before if n.startswith("model/values_fn/"))
        want = outs[u]["metrics"].copy()
        if not pol:      # the last policy update's value (0 before the first)
            prev = [outs[k]["metrics"][2] for k in range(u) if is_policy(first_step, k, delay)]
            want[2] = prev[-1] if prev else 0.0
        close_fwd(m[0], want, "metrics of update %d" % u)
    assert eng.adam_steps() == (ref.t_qf, ref.t_pi) == (N_UPDATES, sum(is_policy(first_step, u, delay) for u in range(N_UPDATES)))
    close_params(eng.get_parameters(), ref, c["lr"], N_UPDATES)
    eng.close()


def check_one_call_equals_six(make, c, delay=2, first_step=1, explicit=False):
    """One call of six updates against six calls of one: parameters, Adam state and metrics bit for bit (device draws unless
    `explicit`)."""
    kw = (lambda u0, u1: dict(idx=c["idx"][u0:u1], eps=c["eps"][u0:u1])) if explicit else (lambda u0, u1: {})
    one = make(c, delay)
    one.train(N_UPDATES, first_step=first_step, **kw(0, N_UPDATES))
    m_one, s_one = one.metrics(), state_of(one)
    one.close()
    six = make(c, delay)
    rows = []
    for u in range(N_UPDATES):
        six.train(1, first_step=first_step + u, **kw(u, u + 1))
        rows.append(six.metrics()[0])
    s_six = state_of(six)
    six.close()
    assert not same_state(s_one, s_six), same_state(s_one, s_six)
    assert same_bits(m_one, np.stack(rows))
    assert np.isfinite(m_one).all()
    return s_one, m_one


def check_policy_loss_is_carried_without_a_fetch(make, c):
    """A critic-only call reports the last policy update's loss whether or not the metrics of the call that made it were read."""
    rows = []
    for fetch in (True, False):
        eng = make(c, 3)
        eng.train(2, c["idx"][:2], c["eps"][:2], first_step=0)      # policy, critic-only
        if fetch:
            first = eng.metrics()
        eng.train(1, c["idx"][2:3], c["eps"][2:3], first_step=2)    # critic-only, a call of its own
        eng.train(2, c["idx"][3:5], c["eps"][3:5], first_step=4)    # critic-only, critic-only
        rows.append(eng.metrics())
        eng.close()
    assert first[0, 5] == 1.0 and first[1, 5] == 0.0 and first[0, 2] != 0.0
    assert same_bits(rows[0], rows[1])
    assert rows[1].shape == (2, 6) and not rows[1][:, 5].any() and same_bits(rows[1][:, 2], np.repeat(first[0, 2], 2))


def launches_per_update(make, c):
    """(critic-only, policy) launches grl_profile_* counts for one update of each kind."""
    eng = make(c, 2)
    n = []
    for first_step in (1, 0):
        eng.profile(True)
        eng.train(1, first_step=first_step)
        eng.synchronize()
        n.append(sum(v["launches"] for v in eng.profile_dump().values()))
        eng.profile(False)
    eng.close()
    return tuple(n)


def planned_launches(plan):
    """(critic-only, policy, policy_delay) of the `grl plan: td3` line of a GRL_PLAN_DUMP text."""
    import re
    lines = sorted(set(l for l in plan.splitlines() if l.startswith("grl plan: td3 ")))      # (sizing and creation both plan)
    assert len(lines) == 1, plan
    m = re.search(r"critic-only update (\d+) launches, policy update (\d+) launches, policy_delay (\d+)", lines[0])
    assert m, lines
    return tuple(int(g) for g in m.groups())
