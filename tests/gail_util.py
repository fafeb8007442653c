"""GAIL on the engine (csrc/plan_gail.inl, csrc/gail_kernels.h) against a float64 restatement of the discriminator.

Nothing in the reference pins GAIL and stable-baselines is not installed, so stable-baselines 2.10.1 `gail/adversary.py`
(TransitionClassifier on Box actions), `common/mpi_running_mean_std.py` and the `using_gail` branches of `trpo_mpi/trpo_mpi.py` are
restated here in torch float64 with autograd, the way they are written there:
    x = [ (obs - mean) / std | action ];  D = W3 tanh(W2 tanh(W1 x + b1) + b2) + b3
    mean = float32(sum / count),  std = sqrt(max(float32(sumsq / count) - mean^2, 1e-2)) formed in float32   (epsilon 1e-2)
    generator_loss = mean softplus(g), expert_loss = mean softplus(-e), ent(x) = (1 - sigmoid(x)) x + softplus(-x),
    total = generator_loss + expert_loss - entcoeff * mean over all logits of ent;  reward = -log(1 - sigmoid(D) + 1e-8)
    per minibatch: obs_rms.update(concat(ob_g, ob_e)), THEN losses and gradient, then TF-1 Adam (0.9 / 0.999 / 1e-8).
The same helpers drive a handle of the emulation build (tests/test_hostemu_gail.py) and of the device (tests/test_gpu_gail.py).

Tolerances are the project's: inputs, logits, rewards and the six diagnostics |d| <= 1e-5 + 1e-4 |ref|; every
gradient tensor within 1e-3 max|g|; parameters after n updates by parity_util.compare_params; float64 sum / sumsq within 1e-12
relative (float64 rounding x a few thousand rows), count exact.  `preconditions` looks at the restatement alone, before anything
is compared: no compared logit within 1e-4 of 0 (the accuracies branch there), and every column that is not constant keeps
E[x^2] <= 4 var after each update, so that the float32 difference E[x^2] - mean^2 keeps five digits.  The seeds below were
searched for on the CPU (`find_seed`); none needs a second look."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import parity_util as pu
import ppo_util
import trpo_util as tu

N_ROWS = 40          # rows of every case's expert table

# obs_dim / A / hidden / T / d_step -> batch = T // d_step, T // batch minibatches per shuffle of the rollout
CASES = {
    # input width 16 after padding, odd hidden; batch 7, three minibatches, one row dropped; a constant observation column (the
    # real image's pad channel); bounds of +-0.5 that the policy's actions exceed; the sixth expert batch of the table is short
    "odd_37": dict(obs_dim=13, A=3, hidden=37, T=22, d_step=3, const_col=5, bound=0.5, seed=0),
    "batch_2": dict(obs_dim=11, A=1, hidden=100, T=8, d_step=3, seed=2),                   # batch 2, FOUR minibatches (seeds 0, 1: a column with E[x^2] > 4 var)
    # two blocks of the 256-row loss launch; every expert batch holds the table's 40 rows of 300: the means use n_e, not batch
    "two_blocks": dict(obs_dim=20, A=2, hidden=16, T=300, d_step=1, seed=0),
    "wide_obs": dict(obs_dim=2310, A=5, hidden=64, T=16, d_step=2, seed=0),                # split-K first layer
}
DEFAULTS = dict(entcoeff=1e-3, d_stepsize=3e-4, bound=1.0, pi=(16,), vf=(8,))


def make_case(name, **over):
    a = dict(DEFAULTS)
    a.update(CASES[name])
    a.update(over)
    c = tu.make_case("odd", seed=a["seed"], obs_dim=a["obs_dim"], A=a["A"], pi=a["pi"], vf=a["vf"], T=a["T"])
    T, od, A = a["T"], a["obs_dim"], a["A"]
    rng = np.random.default_rng(3000 + a["seed"])
    batch = T // a["d_step"]
    c.update(gail_name=name, hidden=a["hidden"], d_step=a["d_step"], batch=batch, n_mb=T // batch, entcoeff=a["entcoeff"],
             d_stepsize=a["d_stepsize"], low=np.full(A, -a["bound"], np.float32), high=np.full(A, a["bound"], np.float32))
    c["exp_obs"] = rng.normal(0.1, 1.2, (N_ROWS, od)).astype(np.float32)
    c["exp_act"] = rng.uniform(-a["bound"], a["bound"], (N_ROWS, A)).astype(np.float32)
    if a.get("const_col") is not None:
        c["obs"] = c["obs"].copy()
        c["obs"][:, a["const_col"]] = 0.5
        c["exp_obs"][:, a["const_col"]] = 0.5
        c["last_obs"] = c["last_obs"].copy()
    c["const_col"] = a.get("const_col")
    # Glorot-uniform weights, zero biases (tf.contrib.layers.fully_connected)
    K, H = od + A, a["hidden"]
    P = OrderedDict()
    for nm, (i, o) in (("fully_connected", (K, H)), ("fully_connected_1", (H, H)), ("fully_connected_2", (H, 1))):
        lim = np.sqrt(6.0 / (i + o))
        P["adversary/%s/weights:0" % nm] = rng.uniform(-lim, lim, (i, o)).astype(np.float32)
        P["adversary/%s/biases:0" % nm] = np.zeros(o, np.float32)
    c["D"] = P
    # shuffles of the rollout (two, or as many as give four updates): n_mb minibatches of `batch` rows each, the tail dropped; the
    # expert rows as the loader hands them out: a permutation of the table per epoch in chunks of `batch`, the last of an epoch
    # shorter (-1 tail)
    shuffles = max(2, -(-4 // c["n_mb"]))
    gen = np.concatenate([rng.permutation(T)[:c["n_mb"] * batch].reshape(c["n_mb"], batch) for _ in range(shuffles)]).astype(np.int32)
    rows, pending = [], []
    while len(rows) < len(gen):
        if not pending:
            perm = rng.permutation(N_ROWS)
            pending = [perm[i:i + batch] for i in range(0, N_ROWS, batch)]
        r = pending.pop(0)
        rows.append(np.concatenate([r, np.full(batch - len(r), -1)]))
    c["gen_idx"], c["exp_idx"] = gen, np.stack(rows).astype(np.int32)
    return c


# --------------------------------------------------------------------------------------------------- the restatement
def softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


class Disc:
    """TransitionClassifier in float64: parameters, running statistics, Adam."""

    def __init__(self, c, P=None):
        self.c = c
        self.P = OrderedDict((n, torch.tensor(np.asarray(a, np.float64))) for n, a in (P or c["D"]).items())
        od = c["obs_dim"]
        self.sum, self.sumsq, self.count = np.zeros(od), np.full(od, 1e-2), 1e-2
        self.m = {n: torch.zeros_like(p) for n, p in self.P.items()}
        self.v = {n: torch.zeros_like(p) for n, p in self.P.items()}
        self.t = 0

    def rms_update(self, x):
        x = np.asarray(x, np.float64)
        self.sum = self.sum + x.sum(axis=0)
        self.sumsq = self.sumsq + np.square(x).sum(axis=0)
        self.count = self.count + len(x)

    def mean_std(self):
        mean = (self.sum / self.count).astype(np.float32)
        var = np.maximum((self.sumsq / self.count).astype(np.float32) - np.square(mean), np.float32(1e-2))
        assert mean.dtype == np.float32 and var.dtype == np.float32
        return mean, np.sqrt(var)

    def x(self, obs, act):
        mean, std = self.mean_std()
        o = (np.asarray(obs, np.float64) - mean.astype(np.float64)) / std.astype(np.float64)
        return torch.tensor(np.concatenate([o, np.asarray(act, np.float64)], axis=1))

    def logits(self, x, P=None):
        P = P or self.P
        n = "adversary/fully_connected%s/%s:0"
        h = torch.tanh(x @ P[n % ("", "weights")] + P[n % ("", "biases")])
        h = torch.tanh(h @ P[n % ("_1", "weights")] + P[n % ("_1", "biases")])
        return (h @ P[n % ("_2", "weights")] + P[n % ("_2", "biases")])[:, 0]

    def rewards(self, obs, act, clip=True):
        if clip:
            act = np.clip(act, self.c["low"], self.c["high"])
        with torch.no_grad():
            d = self.logits(self.x(obs, act))
            return (-torch.log(1.0 - torch.sigmoid(d) + 1e-8)).numpy(), d.numpy()

    def update(self, ob_g, ac_g, ob_e, ac_e, stats_first=True):
        """One minibatch: the input, logits, six diagnostics, gradients; then Adam.  stats_first=False is the WRONG order (losses at
        the statistics from before this minibatch), kept to show that the comparison tells them apart."""
        both = np.concatenate([ob_g, ob_e])
        if stats_first:
            self.rms_update(both)
        P = OrderedDict((n, p.clone().requires_grad_(True)) for n, p in self.P.items())
        x = self.x(both, np.concatenate([ac_g, ac_e]))
        if not stats_first:
            self.rms_update(both)
        d = self.logits(x, P)
        g, e = d[:len(ob_g)], d[len(ob_g):]
        ent = lambda z: (1.0 - torch.sigmoid(z)) * z + softplus(-z)
        gl, el, en = softplus(g).mean(), softplus(-e).mean(), ent(d).mean()
        total = gl + el - self.c["entcoeff"] * en
        grads = OrderedDict(zip(P, torch.autograd.grad(total, list(P.values()))))
        with torch.no_grad():
            losses = [float(gl), float(el), float(en), float(-self.c["entcoeff"] * en), float((torch.sigmoid(g) < 0.5).double().mean()),
                      float((torch.sigmoid(e) > 0.5).double().mean())]
        self.t += 1
        lr = self.c["d_stepsize"] * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t)
        for n in self.P:
            self.m[n] = 0.9 * self.m[n] + 0.1 * grads[n]
            self.v[n] = 0.999 * self.v[n] + 0.001 * grads[n] ** 2
            self.P[n] = self.P[n] - lr * self.m[n] / (torch.sqrt(self.v[n]) + 1e-8)
        return dict(x=x.numpy(), logits=d.detach().numpy(), losses=np.array(losses), grads=OrderedDict((n, v.numpy()) for n, v in grads.items()))

    def check_columns(self, what):
        """every column that is not constant: E[x^2] <= 4 var, so float32 keeps five digits of E[x^2] - mean^2"""
        msq, mean = self.sumsq / self.count, self.sum / self.count
        var = msq - mean ** 2
        for col in range(len(var)):
            if col == self.c["const_col"]:
                assert var[col] < 1e-2, "the constant column is not clamped"
                continue
            assert var[col] > 1e-2 and msq[col] <= 4.0 * var[col], "%s: column %d has E[x^2] %.3e against var %.3e: choose another seed" % (
                what, col, msq[col], var[col])


def minibatch(c, u):
    gi, ei = c["gen_idx"][u], c["exp_idx"][u]
    ei = ei[ei >= 0]
    return c["obs"][gi], c["act"][gi], c["exp_obs"][ei], c["exp_act"][ei]


_REF = {}


def reference(c, n_updates):
    """The restatement's record of updates 0 .. n_updates - 1 and the Disc behind them; computed once per case and left unchanged."""
    key = (c["gail_name"], c["seed"], n_updates)
    if key not in _REF:
        d = Disc(c)
        out = []
        for u in range(n_updates):
            out.append(d.update(*minibatch(c, u)))
            d.check_columns("%s update %d" % (c["gail_name"], u))
            assert np.abs(out[-1]["logits"]).min() > 1e-4, "%s update %d: a logit within 1e-4 of 0: choose another seed" % (c["gail_name"], u)
        _REF[key] = (out, d)
    return _REF[key]


def preconditions(c, n_updates=4):
    reference(c, n_updates)
    if c["gail_name"] == "odd_37":
        assert (np.abs(c["act"]) > c["high"]).any(), "no policy action exceeds the bounds"
        assert (c["exp_idx"][:n_updates + 2] < 0).any(), "no expert batch is short"


def find_seed(name, tries=200):
    for seed in range(tries):
        try:
            c = make_case(name, seed=seed)
            preconditions(c)
            r = Disc(c)
            r.rms_update(c["exp_obs"])
            assert np.abs(r.rewards(c["obs"], c["act"])[1]).min() > 1e-4
            return seed
        except AssertionError:
            continue
    raise AssertionError("no seed")


# --------------------------------------------------------------------------------------------------- the engine
def begin(eng, c, **over):
    eng.gail_begin(over.get("hidden", c["hidden"]), over.get("batch", c["batch"]), c["entcoeff"], c["d_stepsize"], c["low"], c["high"],
                   params=c["D"])
    return eng.gail_upload(c["exp_obs"], c["exp_act"])


def arenas(eng):
    """raw words of the handle's state, replay and work arenas and of the session buffer"""
    out = [np.array(eng.be.to_host(t), copy=True).view(np.uint32) for t in (eng.state, eng.replay, eng.work)]
    if getattr(eng, "_session", None):
        out.append(np.array(eng.be.to_host(eng._session["buf"]), copy=True).view(np.uint32))
    return out


def close_stats(eng, d):
    s, q, n = eng.gail_get_stats()
    assert n == d.count, (n, d.count)
    for a, r, what in ((s, d.sum, "sum"), (q, d.sumsq, "sumsq")):
        assert (np.abs(a - r) <= 1e-12 * np.abs(r)).all(), "%s: max relative deviation %.3e" % (what, (np.abs(a - r) / np.abs(r)).max())


class _Params:
    def __init__(self, P):
        self.P = P


class _EngParams:
    def __init__(self, eng):
        self.get_parameters = eng.gail_get_parameters


def check_updates(eng, c):
    """One update, then three in one call, against the restatement.  Returns the engine's discriminator parameters."""
    preconditions(c)
    out, dref = reference(c, 4)
    b, od, A = c["batch"], c["obs_dim"], c["A"]
    ldx = (od + A + 3) // 4 * 4
    tu.place_and_finish(eng, c)
    table = begin(eng, c)
    assert list(eng.gail_param_shapes().items()) == [(n, p.shape) for n, p in c["D"].items()]
    for n, p in eng.gail_get_parameters().items():
        assert np.array_equal(p, c["D"][n]), n
    eng.gail_update(table, c["gen_idx"][:1], c["exp_idx"][:1])
    r = out[0]
    n_e = int((c["exp_idx"][0] >= 0).sum())
    x = eng.fetch("gail_x", (2 * b, ldx))
    assert not x[:, od + A:].any(), "the padding columns of the input are not zero"
    pu.close(x[:b + n_e, :od + A], r["x"], what="input")
    if c["const_col"] is not None:      # the clamp: std = sqrt(1e-2) in float32, exactly
        mean = first_mean(c)[c["const_col"]]
        assert (x[:b + n_e, c["const_col"]] == (np.float32(0.5) - mean) / np.sqrt(np.float32(1e-2))).all()
    # the statistics are updated BEFORE the loss: the restatement with the other order must fail the same comparison
    wrong = Disc(c).update(*minibatch(c, 0), stats_first=False)
    with pytest.raises(AssertionError):
        pu.close(x[:b + n_e, :od + A], wrong["x"], what="input at the statistics of the previous minibatch")
    with pytest.raises(AssertionError):
        pu.close(eng.fetch("gail_logits", (2 * b,))[:b + n_e], wrong["logits"], what="logits at the statistics of the previous minibatch")
    pu.close(eng.fetch("gail_logits", (2 * b,))[:b + n_e], r["logits"], what="logits")
    assert not eng.fetch("gail_dlogits", (2 * b, 4))[b + n_e:].any(), "an absent row has an output gradient"
    losses = eng.gail_losses()
    assert losses.shape == (1, 6)
    print("losses", losses[0], "reference", r["losses"])
    pu.close(losses[0], r["losses"], what="diagnostics")
    G = eng.gail_get_parameters("gail_grads")
    for n, g in r["grads"].items():
        pu.close_rel_max(G[n], g, what="grad " + n)
    first = Disc(c)
    first.update(*minibatch(c, 0))
    close_stats(eng, first)
    pu.compare_params(_EngParams(eng), _Params(OrderedDict((n, p.numpy()) for n, p in first.P.items())), c["d_stepsize"], 1)
    eng.gail_update(table, c["gen_idx"][1:4], c["exp_idx"][1:4])
    losses = eng.gail_losses()
    assert losses.shape == (3, 6)
    pu.close(losses, np.stack([o["losses"] for o in out[1:4]]), what="diagnostics of updates 1..3")
    close_stats(eng, dref)
    pu.compare_params(_EngParams(eng), _Params(OrderedDict((n, p.numpy()) for n, p in dref.P.items())), c["d_stepsize"], 4)
    P = eng.gail_get_parameters()
    assert all(not np.array_equal(P[n], c["D"][n]) for n in P), "a tensor did not move"
    eng.gail_end()
    return P


def first_mean(c):
    d = Disc(c)
    d.rms_update(np.concatenate([minibatch(c, 0)[0], minibatch(c, 0)[2]]))
    return d.mean_std()[0]


def session_snapshot(eng):
    return [np.asarray(v).view(np.uint32).copy() for blk in ("gail_params", "gail_adam_m", "gail_adam_v") for v in eng.gail_get_parameters(blk).values()] + \
           [np.concatenate([np.ravel(a) for a in eng.gail_get_stats()]).view(np.uint64)]


def check_one_call_equals_single_calls(make_engine, c, n=4):
    snaps = []
    for split in (False, True):
        eng = make_engine()
        tu.place_and_finish(eng, c)
        table = begin(eng, c)
        if split:
            for u in range(n):
                eng.gail_update(table, c["gen_idx"][u:u + 1], c["exp_idx"][u:u + 1])
        else:
            eng.gail_update(table, c["gen_idx"][:n], c["exp_idx"][:n])
        snaps.append(session_snapshot(eng) + [eng.gail_losses()[-1:].view(np.uint32)])
        eng.gail_end()
        eng.close()
    for a, b in zip(*snaps):
        assert np.array_equal(a, b)
    return snaps[0]


def check_second_session_starts_fresh(eng, c):
    tu.place_and_finish(eng, c)
    out = []
    for _ in range(2):
        table = begin(eng, c)
        eng.gail_update(table, c["gen_idx"][:2], c["exp_idx"][:2])
        out.append(session_snapshot(eng))
        eng.gail_end()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def check_rewards(eng, c, trpo_update=True):
    """The reward pass on a full rollout: clipped actions, true rewards kept, GAE from the rewritten rewards bit for bit, and the
    TRPO update behind it against trpo_util's restatement fed those rewards."""
    T, A, od = c["T"], c["A"], c["obs_dim"]
    eng.place_rollout(c["obs"][None], c["act"][None], c["vpred"][None], c["nlp"][None], c["rew"][None], c["es"][None])
    begin(eng, c)
    d = Disc(c)
    d.rms_update(c["exp_obs"])
    d.check_columns(c["gail_name"] + " reward statistics")
    eng.gail_set_stats(d.sum, d.sumsq, d.count)
    close_stats(eng, d)
    want, logit = d.rewards(c["obs"], c["act"])
    assert np.abs(logit).min() > 1e-4
    eng.gail_rewards()
    ldx = (od + A + 3) // 4 * 4
    x = eng.fetch("gail_rew_x", (T, ldx))
    assert np.array_equal(x[:, od:od + A], np.clip(c["act"], c["low"], c["high"])), "the reward pass does not see the clipped actions"
    pu.close(eng.fetch("gail_rew_logits", (T,)), logit, what="logits of the rollout")
    rew = eng.fetch("ppo_rew", (T,))
    pu.close(rew, want, what="rewards")
    if (np.abs(c["act"]) > c["high"]).any():
        with pytest.raises(AssertionError):
            pu.close(rew, d.rewards(c["obs"], c["act"], clip=False)[0], what="rewards on unclipped actions")
    assert np.array_equal(eng.fetch("gail_true_rew", (T,)).view(np.uint32), c["rew"].view(np.uint32)), "the environment's rewards are not kept"
    eng.finish(c["last_obs"], [c["last_es"]])
    last_v = eng.fetch("ppo_last_v", (1,))
    adv, ret = ppo_util.gae_np(rew[None], c["vpred"][None], c["es"][None], last_v, np.array([c["last_es"]], np.float32), c["gamma"], c["lam"])
    assert np.array_equal(eng.fetch("ppo_adv", (T,)).view(np.uint32), adv[0].view(np.uint32))
    assert np.array_equal(eng.fetch("ppo_ret", (T,)).view(np.uint32), ret[0].view(np.uint32))
    if trpo_update:
        c2 = dict(c, rew=rew)
        o64, m = tu.check_update(eng, c2)      # (places the same rollout with the rewritten rewards: the same GAE, then the update)
        assert np.array_equal(eng.fetch("ppo_adv", (T,)).view(np.uint32), adv[0].view(np.uint32))
    eng.gail_end()


def check_update_reads_unclipped_actions(eng, c):
    """the generator rows of an update are the policy's actions as stored, beyond the bounds"""
    assert (np.abs(c["act"]) > c["high"]).any()
    tu.place_and_finish(eng, c)
    table = begin(eng, c)
    eng.gail_update(table, c["gen_idx"][:1], c["exp_idx"][:1])
    b, od, A = c["batch"], c["obs_dim"], c["A"]
    x = eng.fetch("gail_x", (2 * b, (od + A + 3) // 4 * 4))
    got = x[:b, od:od + A]
    assert np.array_equal(got, c["act"][c["gen_idx"][0]]) and (np.abs(got) > c["high"]).any()
    eng.gail_end()


def check_state_rules(eng, c):
    """every GRL_ERR_STATE / GRL_ERR_INVALID of a TRPO handle's GAIL calls, by message; nothing moves"""
    from grasp_rl._capi import GrlError
    T, b = c["T"], c["batch"]
    eng.place_rollout(c["obs"][None], c["act"][None], c["vpred"][None], c["nlp"][None], c["rew"][None], c["es"][None])
    before = arenas(eng)
    for call, name in ((eng.gail_rewards, "grl_gail_rewards"), (eng.gail_losses, "grl_gail_get_losses"), (eng.gail_get_stats, "grl_gail_get_stats"),
                       (eng.gail_end, "grl_gail_end")):
        with pytest.raises(GrlError, match=name + " needs an open session"):
            call()
    with pytest.raises(GrlError, match=r"hidden must be 1..1024 \(1025\)"):
        begin(eng, c, hidden=1025)
    with pytest.raises(GrlError, match=r"batch %d is outside 1..%d" % (T + 1, T)):
        begin(eng, c, batch=T + 1)
    assert all(np.array_equal(x, y) for x, y in zip(before, arenas(eng))), "a refused call moved something"
    table = begin(eng, c)
    before = arenas(eng)
    with pytest.raises(GrlError, match="a GAIL session is open"):
        begin(eng, c)
    with pytest.raises(GrlError, match="none is held"):
        eng.gail_update(table, c["gen_idx"][:1], c["exp_idx"][:1])      # the rollout is full but not finished
    eng.gail_rewards()
    after_rewards = arenas(eng)
    with pytest.raises(GrlError, match="the discriminator's already"):
        eng.gail_rewards()
    eng.finish(c["last_obs"], [c["last_es"]])
    with pytest.raises(GrlError, match="has not closed yet"):
        eng.gail_rewards()
    mid = arenas(eng)
    for what, row, col, val, msg in (("gen", 1, 2, T, "generator index of update 1, entry 2 is outside the rollout"),
                                     ("gen", 0, 0, -1, "generator index of update 0, entry 0 is outside the rollout"),
                                     ("exp", 1, 1, N_ROWS, "expert index of update 1, entry 1 is outside the table"),
                                     ("exp", 0, 0, -1, "expert index of update 0, entry 0: a minibatch needs at least one row")):
        gi, ei = c["gen_idx"][:2].copy(), c["exp_idx"][:2].copy()
        (gi if what == "gen" else ei)[row, col] = val
        with pytest.raises(GrlError, match=msg):
            eng.gail_update(table, gi, ei)
    if b >= 3:
        ei = c["exp_idx"][:2].copy()
        ei[1, 1] = -1
        ei[1, 2] = 0
        with pytest.raises(GrlError, match="expert index of update 1, entry 2 follows a -1"):
            eng.gail_update(table, c["gen_idx"][:2], ei)
    with pytest.raises(GrlError, match="count of a call must be 1..4096"):
        eng.gail_update(table, np.zeros((0, b), np.int32), np.zeros((0, b), np.int32))
    assert all(np.array_equal(x, y) for x, y in zip(mid, arenas(eng))), "a refused call moved something"
    # valid whether or not the TRPO update ran in between, until the next step writes a slot
    eng.update(c["vf_perm"])
    eng.gail_update(table, c["gen_idx"][:1], c["exp_idx"][:1])
    eng.step(c["obs"][0], [c["es"][0]], c["eps"][0])
    held = arenas(eng)
    with pytest.raises(GrlError, match="none is held"):
        eng.gail_update(table, c["gen_idx"][:1], c["exp_idx"][:1])
    assert all(np.array_equal(x, y) for x, y in zip(held, arenas(eng))), "a refused call moved something"
    assert not np.array_equal(before[1], after_rewards[1])      # (the reward pass did rewrite the rollout's rewards)
    eng.gail_end()


def check_session_leaves_the_handle_alone(make_engine, c, capfd):
    """a TRPO handle with a session open exports the same state bytes, holds the same state and replay arenas after the same TRPO
    update and prints the same TRPO plan lines as one without"""
    res = []
    for session in (False, True):
        capfd.readouterr()
        eng = make_engine()
        tu.place_and_finish(eng, c)
        if session:      # (the work arena holds launch tables with addresses: it is compared on the one handle)
            work = arenas(eng)[2]
            table = begin(eng, c)
            eng.gail_update(table, c["gen_idx"][:2], c["exp_idx"][:2])
            assert np.array_equal(work, arenas(eng)[2]), "the session moved the handle's work arena"
        blob = eng.export_state()
        eng.update(c["vf_perm"])
        ar = arenas(eng)[:2]
        lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("grl plan:")]
        if session:
            assert any(l.startswith("grl plan: gail rewards ") for l in lines) and any(l.startswith("grl plan: gail update ") for l in lines)
            eng.gail_end()
        res.append((blob, ar, [l for l in lines if l.startswith(("grl plan: trpo", "grl plan: ppo"))]))
        eng.close()
    assert res[0][0] == res[1][0], "the exported state differs"
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1])), "an arena of the handle differs"
    assert res[0][2] == res[1][2] and len(res[0][2]) > 3, "the TRPO plan lines differ"


def routes_from_dump(text):
    """{pass: (launches, first-layer route)} from the two `grl plan: gail ...` lines"""
    import re
    out = {}
    for kind, n, route in re.findall(r"grl plan: gail (rewards|update) +(\d+) launches.*first layer (whole|split \d+)", text):
        out[kind] = (int(n), route)
    return out


def check_foreign_handles_refuse(lib, handles):
    import ctypes as C
    n, d = C.c_size_t(), C.c_double()
    for h in handles:
        for call, what in ((lambda: lib.grl_gail_query_sizes(h, None, C.byref(n)), b"grl_gail_query_sizes"),
                           (lambda: lib.grl_gail_begin(h, None, None), b"grl_gail_begin"),
                           (lambda: lib.grl_gail_param_info(h, 0, None, 0, None, None, None, None), b"grl_gail_param_info"),
                           (lambda: lib.grl_gail_rewards(h), b"grl_gail_rewards"),
                           (lambda: lib.grl_gail_update(h, None, None, 0, None, None, 1), b"grl_gail_update"),
                           (lambda: lib.grl_gail_get_losses(h, None, 0), b"grl_gail_get_losses"),
                           (lambda: lib.grl_gail_get_stats(h, None, None, C.byref(d)), b"grl_gail_get_stats"),
                           (lambda: lib.grl_gail_set_stats(h, None, None, 1.0), b"grl_gail_set_stats"),
                           (lambda: lib.grl_gail_end(h), b"grl_gail_end")):
            assert call() == -3                                     # GRL_ERR_STATE
            assert lib.grl_last_error() == what + b" is defined for TRPO handles (grl_trpo_create)"
