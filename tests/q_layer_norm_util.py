"""Layer-normalised DQN / BDQ (grl_config.q_layer_norm, csrc/ln_kernels.h) against a float64 restatement of the Q update.

oracle/dqn.py knows no layer normalisation, so the update is restated here in torch float64 with autograd: dueling combine,
double-Q, Huber / squared loss, BDQ's branch mean and trunk rescaling, per-variable clip_by_norm and TF Adam, plus
tf.contrib.layers.layer_norm (statistics over the layer's width, biased variance, epsilon 1e-12) in front of every HIDDEN layer's
ReLU.  tests/test_hostemu_q_layer_norm.py first holds the restatement, with layer norm off, against oracle/dqn.py's own update
run in float64; only then is it used with layer norm on, by that file (emulation build) and tests/test_gpu_q_layer_norm.py.

Tolerances are the project's: forward |d| <= 1e-5 + 1e-4 |ref|, every gradient tensor within 1e-3 max|g|, one
optimiser step on identical inputs 1e-6.  The seeds below are fixed so that in the float64 reference NO normalised
pre-activation of a differentiated pass lies within 1e-5 of zero (`assert_no_sign_ambiguity`, on the reference alone, before
anything is compared): no ReLU unit is sign-ambiguous and no case is excluded."""
from collections import OrderedDict

import numpy as np
import torch

import parity_util as pu
import q_parity_util as qu
from grasp_rl import _capi
from grasp_rl.engine import QEngine
from oracle import dqn as od

Y_MARGIN = 1e-5          # no normalised pre-activation of the reference closer to zero than this
ACT_GAP = 1e-4           # act rows: top-two gap of the reference's Q-values, every (row, branch)

# shape -> make_q_case arguments + the seed for which the conditions above hold (found by `find_seed`, asserted by every test)
LN_CASES = {
    "dqn_64_64": dict(algo="dqn", obs_dim=20, D=1, bins=6, common=(), branch=(64, 64), value=(64, 64), B=32, seed=1),
    "dqn_48": dict(algo="dqn", obs_dim=13, D=1, bins=5, common=(), branch=(48,), value=(48,), B=17, seed=0),          # tail lanes, tail rows
    "dqn_100_65": dict(algo="dqn", obs_dim=13, D=1, bins=5, common=(), branch=(100, 65), value=(100, 65), B=17, seed=1),
    # the shipped BDQ shape (trained_models/BDQ_33pads_big): 8 elements per lane at width 512
    "bdq_shipped": dict(algo="bdq", obs_dim=100, D=4, bins=33, common=(512, 256), branch=(128,), value=(128,), B=64, seed=0),
    "bdq_no_trunk": dict(algo="bdq", obs_dim=20, D=3, bins=5, common=(), branch=(24, 16), value=(40,), B=9, seed=0),
}
N_STEPS = 3


def _ln(k):
    return "LayerNorm" if k == 0 else "LayerNorm_%d" % k


def ln_param_shapes(spec, layer_norm=True):
    """The parameter table with layer normalisation: oracle/dqn.py's, and behind every HIDDEN layer's weights / biases
    `LayerNorm[_k]/beta:0` then `LayerNorm[_k]/gamma:0` in the layer's scope (TF creation order; k counts per scope)."""
    if not layer_norm:
        return od.param_shapes(spec)
    out = OrderedDict()
    out["%s/eps:0" % spec.scope] = ()
    for prefix in ("%s/model" % spec.scope, "%s/target_q_func/model" % spec.scope):
        count = {}
        for name, shp in od.net_shapes(spec, prefix).items():
            out[name] = shp
            scope = name.rsplit("/", 2)[0]
            out_layer = _is_out(spec, name)
            if name.endswith("biases:0") and not out_layer:
                k = count.get(scope, 0)
                count[scope] = k + 1
                out["%s/%s/beta:0" % (scope, _ln(k))] = shp
                out["%s/%s/gamma:0" % (scope, _ln(k))] = shp
    return out


def _fc_index(name):
    return int(name.split("fully_connected")[1].split("/")[0].lstrip("_") or 0)


def _is_out(spec, name):
    k = _fc_index(name)
    if "/action_value/" in name:
        return k % (len(spec.branch_hidden) + 1) == len(spec.branch_hidden)
    if "/state_value/" in name:
        return k == len(spec.value_hidden)
    return False


def init_ln_params(spec, seed, layer_norm=True):
    """Seeded parameters in which everything takes part: Xavier weights, biases and betas away from zero, gammas around one,
    a target network that differs from the online one."""
    rng = np.random.default_rng(seed)
    P = OrderedDict()
    for name, shp in ln_param_shapes(spec, layer_norm).items():
        if name.endswith("eps:0"):
            P[name] = np.float32(0.0).reshape(())
        elif name.endswith("weights:0"):
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
            P[name] = rng.uniform(-lim, lim, shp).astype(np.float32)
        elif name.endswith("gamma:0"):
            P[name] = rng.uniform(0.5, 1.5, shp).astype(np.float32)
        elif name.endswith("beta:0"):
            P[name] = rng.uniform(-0.2, 0.2, shp).astype(np.float32)
        else:
            P[name] = rng.uniform(-0.1, 0.1, shp).astype(np.float32)
    return P


def forward64(spec, T, prefix, obs, trunk_scale=1.0, layer_norm=True, ys=None):
    """q [B, D, n], float64.  ys: list that receives every normalised pre-activation y (before the ReLU)."""
    count = {}

    def hidden(scope, k, x):
        u = x @ T["%s/%s/%s/weights:0" % (prefix, scope, od._fc(k))] + T["%s/%s/%s/biases:0" % (prefix, scope, od._fc(k))]
        if layer_norm:
            j = count.get(scope, 0)
            count[scope] = j + 1
            mean = u.mean(dim=1, keepdim=True)
            var = ((u - mean) ** 2).mean(dim=1, keepdim=True)               # tf.nn.moments: biased
            u = (u - mean) * torch.rsqrt(var + 1e-12) * T["%s/%s/%s/gamma:0" % (prefix, scope, _ln(j))] \
                + T["%s/%s/%s/beta:0" % (prefix, scope, _ln(j))]
            if ys is not None:
                ys.append(u.detach())
        return torch.relu(u)

    def out(scope, k, x):
        return x @ T["%s/%s/%s/weights:0" % (prefix, scope, od._fc(k))] + T["%s/%s/%s/biases:0" % (prefix, scope, od._fc(k))]

    h = obs
    for k in range(len(spec.common)):
        h = hidden("common_net", k, h)
    if trunk_scale != 1.0:
        h = h * trunk_scale + (h * (1.0 - trunk_scale)).detach()
    advs, k = [], 0
    for _ in range(spec.n_branches):
        z = h
        for _h in spec.branch_hidden:
            z = hidden("action_value", k, z)
            k += 1
        advs.append(out("action_value", k, z))
        k += 1
    adv = torch.stack(advs, dim=1)
    z, k = h, 0
    for _h in spec.value_hidden:
        z = hidden("state_value", k, z)
        k += 1
    v = out("state_value", k, z).reshape(-1)
    return v[:, None, None] + adv - adv.mean(dim=2, keepdim=True)


def clip_adam64(P, G, m, v, t, lr, clip=10.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.clip_by_norm per variable, then TF 1.x ApplyAdam at step t (1-based), float64; updates P, m, v in place."""
    alpha = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    for n, g in G.items():
        g = np.asarray(g, np.float64)
        if clip > 0:
            g = g * clip / max(np.sqrt(np.sum(g * g)), clip)
        m[n] = m[n] + (g - m[n]) * (1.0 - beta1)
        v[n] = v[n] + (g * g - v[n]) * (1.0 - beta2)
        P[n] = P[n] - m[n] * alpha / (np.sqrt(v[n]) + eps)


class QRef64:
    def __init__(self, spec, params, layer_norm=True):
        self.spec, self.layer_norm = spec, layer_norm
        self.P64 = OrderedDict((k, np.array(v, np.float64)) for k, v in params.items())
        self.train_names = [n for n in self.P64 if "/target_q_func/" not in n and not n.endswith("eps:0")]
        self.m = {n: np.zeros_like(self.P64[n]) for n in self.train_names}
        self.v = {n: np.zeros_like(self.P64[n]) for n in self.train_names}
        self.t = 0

    @property
    def P(self):
        return OrderedDict((k, v.astype(np.float32)) for k, v in self.P64.items())

    def _tensors(self, grad=False):
        T = OrderedDict()
        for k, v in self.P64.items():
            T[k] = torch.from_numpy(v.copy())
            if grad and k in self.train_names:
                T[k].requires_grad_(True)
        return T

    def q_values(self, obs):
        return forward64(self.spec, self._tensors(), "%s/model" % self.spec.scope,
                         torch.from_numpy(np.asarray(obs, np.float64)), layer_norm=self.layer_norm).numpy()

    def grads(self, batch, weights):
        spec = self.spec
        T = self._tensors(grad=True)
        b = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in batch.items()}
        w = torch.from_numpy(np.asarray(weights, np.float64))
        pre, ys = "%s/model" % spec.scope, []
        q = forward64(spec, T, pre, b["obs"], spec.trunk_scale, self.layer_norm, ys)
        a = b["act"].long()
        q_sel = torch.gather(q, 2, a[:, :, None]).squeeze(2)
        with torch.no_grad():
            q1 = forward64(spec, T, pre, b["next_obs"], layer_norm=self.layer_norm)
            q2 = forward64(spec, T, "%s/target_q_func/model" % spec.scope, b["next_obs"], layer_norm=self.layer_norm)
            sel = (q1 if spec.double_q else q2).argmax(dim=2)
            q_best = torch.gather(q2, 2, sel[:, :, None]).squeeze(2).mean(dim=1)
            y = b["rew"] + spec.gamma * (1.0 - b["done"]) * q_best
        td = q_sel - y[:, None]
        err = torch.where(td.abs() < 1.0, 0.5 * td ** 2, td.abs() - 0.5) if spec.huber else td ** 2
        loss = torch.mean(w * (err.sum(dim=1) if (spec.algo == "bdq" and spec.loss_sum_branches) else err.mean(dim=1)))
        gs = torch.autograd.grad(loss, [T[n] for n in self.train_names])
        G = {n: g.numpy().copy() for n, g in zip(self.train_names, gs)}
        min_y = min((float(yy.abs().min()) for yy in ys), default=np.inf)
        return {"loss": float(loss.detach()), "td": td.detach().numpy(), "q": q.detach().numpy(),
                "priority": td.detach().abs().sum(dim=1).numpy(), "min_abs_y": min_y, "grads": G}

    def step(self, batch, weights):
        out = self.grads(batch, weights)
        self.t += 1
        clip_adam64(self.P64, out["grads"], self.m, self.v, self.t, self.spec.lr, self.spec.grad_clip)
        return out

    def update_target(self):
        for n in self.P64:
            if "/target_q_func/" in n:
                self.P64[n] = self.P64[n.replace("/target_q_func", "")].copy()


def make_ln_case(name, layer_norm=True, **over):
    """make_q_case of an LN_CASES shape with standard-normal observations (pre-activation rows of variance of order one, never
    constant), the parameters of init_ln_params and q_layer_norm set."""
    a = dict(LN_CASES[name])
    a.update(over)
    seed = a.pop("seed")
    case = qu.make_q_case(seed=seed, n_steps=N_STEPS, **a)
    rng = np.random.default_rng(1000 + seed)
    n = case["tr"]["obs"].shape
    case["tr"]["obs"] = rng.normal(0.0, 1.0, n).astype(np.float32)
    case["tr"]["next_obs"] = rng.normal(0.0, 1.0, n).astype(np.float32)
    case["cfg"].q_layer_norm = 1 if layer_norm else 0
    case["params"] = init_ln_params(case["spec"], seed, layer_norm)
    case["layer_norm"] = layer_norm
    return case


def batch_of(case, s):
    tr, ii = case["tr"], case["idx"][s]
    return {k: tr[k][ii] for k in ("obs", "next_obs", "act", "rew", "done")}


def reference_run(case):
    """The float64 trajectory of the case's N_STEPS updates: [per-step outputs], the reference after them."""
    ref = QRef64(case["spec"], case["params"], case["layer_norm"])
    return [ref.step(batch_of(case, s), case["weights"][s]) for s in range(case["n_steps"])], ref


def assert_no_sign_ambiguity(steps):
    for s, out in enumerate(steps):
        assert out["min_abs_y"] > Y_MARGIN, "step %d: a normalised pre-activation of the reference lies %.2e from zero" % (s, out["min_abs_y"])


def find_seed(name, tries=200):
    """(development aid) the first seed of an LN_CASES shape that satisfies assert_no_sign_ambiguity and act_rows' gap"""
    for seed in range(tries):
        case = make_ln_case(name, seed=seed)
        steps, _ = reference_run(case)
        if min(o["min_abs_y"] for o in steps) > Y_MARGIN and all(_act_gap_ok(case, n) for n in qu.ACT_NS):
            return seed
    return None


def act_rows(case, n):
    return np.random.default_rng(500 + n).normal(0.0, 1.0, (n, case["spec"].obs_dim)).astype(np.float32)


def _act_gap_ok(case, n):
    q = QRef64(case["spec"], case["params"], case["layer_norm"]).q_values(act_rows(case, n))
    top = np.sort(q, axis=2)[:, :, -2:]
    return bool(((top[:, :, 1] - top[:, :, 0]) > ACT_GAP).all())


def engine_setup(case, backend=None, lib_path=None, act_batch=None):
    if act_batch is not None:
        case["cfg"].act_batch = act_batch
    return qu.q_engine_setup(case, backend, lib_path)


def run_and_compare_ln(case, backend=None, lib_path=None):
    """Forward, gradients, one optimiser step on identical inputs and the N_STEPS-update trajectory of a layer-normalised
    handle against the float64 reference; then the target copy."""
    spec = case["spec"]
    steps, ref_end = reference_run(case)
    assert_no_sign_ambiguity(steps)                       # on the reference alone, before anything is compared
    ref0 = QRef64(spec, case["params"], case["layer_norm"])
    eng = engine_setup(case, backend, lib_path)
    try:
        table = [(t[0], tuple(t[3])) for t in eng.table]
        assert table == [(k, tuple(v)) for k, v in ln_param_shapes(spec, case["layer_norm"]).items()]
        obs4 = case["tr"]["obs"][:4]
        pu.close(eng.q_values(obs4), ref0.q_values(obs4), atol=1e-5, rtol=1e-4, what="Q-values (act path)")
        for s in range(case["n_steps"]):
            ref = steps[s]
            eng.compute_grads(case["idx"][s:s + 1], case["weights"][s:s + 1])
            pu.close(eng.td_errors(), ref["td"], atol=1e-5, rtol=1e-4, what="td step %d" % s)
            if s == 0:
                G = eng.get_gradients()
                assert set(G) >= set(ref["grads"])
                for n, g in ref["grads"].items():
                    print("grad %-60s max|d| %.3e  max|g| %.3e" % (n, np.abs(G[n] - g).max(), np.abs(g).max()))
                    pu.close_rel_max(G[n], g, rel=1e-3, what="grad " + n)
                assert abs(eng.metrics()["policy_loss"] - ref["loss"]) <= 1e-4 * abs(ref["loss"]) + 1e-6
                # one optimiser step on identical inputs: the engine's own parameters, gradients and moments through the
                # float64 clip + Adam
                P0 = OrderedDict((k, np.asarray(v, np.float64)) for k, v in eng.get_parameters().items())
                m0, v0 = pu.adam_state(eng)
                m = {n: np.asarray(m0[n], np.float64) for n in G if n in ref["grads"]}
                v = {n: np.asarray(v0[n], np.float64) for n in G if n in ref["grads"]}
                clip_adam64(P0, {n: G[n] for n in ref["grads"]}, m, v, 1, spec.lr, spec.grad_clip)
                eng.apply_grads(1.0)
                P1 = eng.get_parameters()
                for n in ref["grads"]:
                    d = np.abs(np.asarray(P1[n], np.float64) - P0[n]).max()
                    assert d <= 1e-6, "optimiser step %s: max |d| %.3e" % (n, d)
            else:
                eng.apply_grads(1.0)
        pu.compare_params(eng, ref_end, spec.lr, case["n_steps"])
        P = eng.get_parameters()
        moved = [n for n in P if n.endswith(("gamma:0", "beta:0")) and "/target_q_func/" not in n
                 and not np.array_equal(P[n], case["params"][n])]
        assert not case["layer_norm"] or len(moved) == sum(n.endswith(("gamma:0", "beta:0")) for n in ref_end.train_names)
        eng.update_target()
        P = eng.get_parameters()
        for n in P:
            if "/target_q_func/" in n:
                assert np.array_equal(P[n], P[n.replace("/target_q_func", "")]), n
    finally:
        eng.close()


def act_check(case, n, backend=None, lib_path=None):
    """grl_act(GRL_ACT_GREEDY) on n rows == the arg-max of the reference's Q-values; every (row, branch) has a top-two gap above
    ACT_GAP in float64 (asserted first), so every one is compared."""
    obs = act_rows(case, n)
    q = QRef64(case["spec"], case["params"], case["layer_norm"]).q_values(obs)
    top = np.sort(q, axis=2)[:, :, -2:]
    assert ((top[:, :, 1] - top[:, :, 0]) > ACT_GAP).all()
    eng = engine_setup(case, backend, lib_path, act_batch=n)
    try:
        bins = eng.act_bins(obs)
        assert np.array_equal(bins, q.argmax(axis=2))
        pu.close(eng.q_values(obs), q, atol=1e-5, rtol=1e-4, what="Q-values")
        assert np.array_equal(eng.act_bins(obs[:1]), bins[:1]) and np.array_equal(eng.act_bins(obs), bins)
    finally:
        eng.close()


def multi_update_check(name, prioritised, backend=None, lib_path=None, n=5, n_store=300):
    """ONE call of n updates on the device RNG == n calls of one update, bit for bit: parameters, Adam moments, drawn indices."""
    def run(split):
        case = make_ln_case(name, n_replay=n_store)
        if prioritised:
            c = case["cfg"]
            c.q_per, c.q_per_alpha, c.q_per_eps, c.q_per_alpha64 = 1, 0.6, 1e-6, 0.6
        eng = engine_setup(case, backend, lib_path)
        for k in split:
            eng.train_per(k, 0.7) if prioritised else eng.train_device(k)
        out = (eng.get_parameters(), eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy(), eng.sampled_indices(), eng.metrics())
        eng.close()
        return out
    ref = run([1] * n)
    for got in (run([n]), run([2, n - 2])):
        for k in ref[0]:
            assert np.array_equal(ref[0][k], got[0][k]), k
        assert np.array_equal(ref[1], got[1]) and np.array_equal(ref[2], got[2])
        assert np.array_equal(ref[3], got[3]) and ref[4] == got[4]
    gam = [k for k in ref[0] if k.endswith("gamma:0") and "/target_q_func/" not in k]
    assert gam and any(not np.array_equal(ref[0][k], make_ln_case(name, n_replay=n_store)["params"][k]) for k in gam)
