"""Wide DQN / BDQ handles (an MLP over a flattened image: a trainable variable of more than 131 072 floats) -- the cases, the
reference and the comparisons shared by tests/test_hostemu_q_wide.py (emulation build) and tests/test_gpu_q_wide.py (MI355X).

Reference and tolerance.  Sums over K = 8192 ... 20 480 taken in another order no longer sit inside tolerances that were fixed for
K <= 300, so the wide cases carry a yardstick of their own:

  * the reference is the float64 restatement of tests/q_layer_norm_util.py (QRef64; layer norm off, or on for that one case);
  * d_ref is the deviation of a float32 step from that float64 run ON THE SAME INPUTS: oracle/dqn.py's own float32 update --
    and, for the layer-normalised case, which oracle/dqn.py cannot express, the same restatement evaluated in float32 (Ref32);
  * the engine may deviate from float64 by the EXISTING per-quantity tolerance (those of q_parity_util.run_and_compare) plus
    4 x d_ref: two float32-faithful summation orders err independently (2 x), and 2 x is headroom for the grouping of the
    layer-0 partial sums.

d_ref and the engine's deviation are printed per case and quantity.  Before anything is compared, the float64 reference alone is
asserted to hold no hidden pre-activation within 1e-3 x max|pre-activation| of zero, in any pass of any update: no ReLU unit is
sign-ambiguous, and no unit, row or case is left out.  Random data cannot satisfy that at 10^4 ... 10^5 pre-activations per
update, so the cases are BUILT for it: every hidden unit's kernel column and bias are set so that its pre-activation over the
replay rows has one common standard deviation t and a mean of +-BIAS_K t (layer norm: beta = +-BIAS_K gamma), which leaves a
unit on or off for all rows while both states occur in every layer; the seeds below are those for which the condition holds
through all three updates (found by `find_seed` on the CPU, asserted by every test)."""
from collections import OrderedDict

import numpy as np
import torch

import parity_util as pu
import q_layer_norm_util as ql
import q_parity_util as qu
from oracle import dqn as od

N_STEPS = 3
MARGIN_REL = 1e-3           # no hidden pre-activation of the reference within this x max|pre-activation| of zero
BIAS_K = 6.0                # hidden units: mean pre-activation +-BIAS_K standard deviations (over the replay rows) from zero
ACT_GAP = 1e-4              # act rows: top-two gap of the reference's Q-values, every (row, branch)
ACT_NS = (1, 16, 17)
WIDE_MIN = 131072           # csrc/q_wide_kernels.h QW_WIDE_MIN: wide = a trainable variable with MORE floats
TILE = 4096                 # csrc/q_wide_kernels.h QW_TILE

_DQN = dict(algo="dqn", D=1, bins=12, common=(), branch=(64, 64), value=(64, 64), lr=5e-4)
# inputs "pixels": integers 0 ... 255 as the image env hands them out (not divided by 255), rewards N(0, 2): the per-variable
#   clip is ACTIVE (scale < 1, asserted on the reference).  lr 1e-6: one Adam step moves every weight by ~lr, so a layer-0
#   pre-activation by up to lr x sum|x| ~ 1e6 lr -- at the stock 5e-4 three updates would carry every unit across zero.
# inputs "normal": N(0, 1), rewards N(0, 0.05), output layers scaled by 0.002: every clip scale is EXACTLY 1 (asserted).
WIDE_CASES = {
    "dqn8192_B32": dict(_DQN, obs_dim=8192, B=32, n_replay=48, inputs="pixels", lr=1e-6, seed=0),
    "dqn8192_B1": dict(_DQN, obs_dim=8192, B=1, n_replay=40, inputs="normal", seed=2),
    "dqn8192_B50": dict(_DQN, obs_dim=8192, B=50, n_replay=64, inputs="normal", seed=0),
    "bdq8192_B16": dict(algo="bdq", obs_dim=8192, D=4, bins=33, common=(64, 64), branch=(32,), value=(32,), B=16, n_replay=40,
                        lr=1e-4, inputs="normal", seed=1),
    "dqn20480": dict(_DQN, obs_dim=20480, B=16, n_replay=40, inputs="pixels", lr=1e-6, seed=0),       # RGB-D: 64 x 64 x 5
    "dqn8192_ln": dict(_DQN, obs_dim=8192, B=16, n_replay=40, inputs="normal", layer_norm=True, seed=0),
    "dqn8192_per": dict(_DQN, obs_dim=8192, B=16, n_replay=64, inputs="normal", per=True, seed=1),
}
PARITY_CASES = [n for n in WIDE_CASES if not WIDE_CASES[n].get("per")]
# the two sides of the route's threshold: 2048 x 64 == 131 072 floats is not wide, 2049 x 64 is (ldf padded to 2052)
EDGE = dict(_DQN, B=8, n_replay=16, inputs="normal", seed=0)


# --------------------------------------------------------------------------------------------------- the float64 reference
def _layers(spec):
    """(scope, index, is_hidden, tower) of every dense layer in creation order; tower: 'c' trunk, branch number, 'v' value"""
    out = [("common_net", k, True, "c") for k in range(len(spec.common))]
    k = 0
    for br in range(spec.n_branches):
        for _ in spec.branch_hidden:
            out.append(("action_value", k, True, br))
            k += 1
        out.append(("action_value", k, False, br))
        k += 1
    out += [("state_value", k, True, "v") for k in range(len(spec.value_hidden))]
    out.append(("state_value", len(spec.value_hidden), False, "v"))
    return out


def hidden_preacts(spec, P, prefix, x, layer_norm, calibrate=None):
    """Every hidden layer's input to its ReLU (layer norm: the normalised, scaled and shifted one) of the network `prefix` on
    rows x, float64.  calibrate (a Generator): first give every hidden unit a pre-activation of mean +-BIAS_K t and standard
    deviation t over the rows x (layer norm: beta = +-BIAS_K gamma), in P."""
    x = np.asarray(x, np.float64)
    pres, h, ln_count, z, scale = [], None, {}, {}, {}
    for scope, k, hidden, tower in _layers(spec):
        base = "%s/%s/%s" % (prefix, scope, od._fc(k))
        src = x if tower == "c" and k == 0 else z.get(tower, h if h is not None else x)
        u = src @ np.asarray(P[base + "/weights:0"], np.float64)
        if not hidden:
            continue
        if layer_norm:
            j = ln_count.get(scope, 0)
            ln_count[scope] = j + 1
            lnb = "%s/%s/%s" % (prefix, scope, ql._ln(j))
            u = u + np.asarray(P[base + "/biases:0"], np.float64)
            mean = u.mean(axis=1, keepdims=True)
            xhat = (u - mean) / np.sqrt(((u - mean) ** 2).mean(axis=1, keepdims=True) + 1e-12)
            gam = np.asarray(P[lnb + "/gamma:0"], np.float64)
            if calibrate is not None:
                P[lnb + "/beta:0"] = (calibrate.choice([-1.0, 1.0], gam.shape) * BIAS_K * gam).astype(np.float32)
            pre = xhat * gam + np.asarray(P[lnb + "/beta:0"], np.float64)
        else:
            if calibrate is not None:
                # every unit's pre-activation over the rows: standard deviation t (the first layer's median, for all layers of
                # the network: the margin is relative to the LARGEST pre-activation), mean +-BIAS_K t
                std = u.std(axis=0)
                t = scale.setdefault("t", float(np.median(std)))
                P[base + "/weights:0"] = (np.asarray(P[base + "/weights:0"], np.float64) * (t / std)).astype(np.float32)
                u = src @ np.asarray(P[base + "/weights:0"], np.float64)
                P[base + "/biases:0"] = (calibrate.choice([-1.0, 1.0], u.shape[1]) * BIAS_K * t - u.mean(axis=0)).astype(np.float32)
            pre = u + np.asarray(P[base + "/biases:0"], np.float64)
        pres.append(pre)
        out = np.maximum(pre, 0.0)
        if tower == "c":
            h = out
        else:
            z[tower] = out
    return pres


def margin(spec, P, batch, layer_norm):
    """min |pre-activation| / max |pre-activation| over the three passes of one update at parameters P"""
    sc = spec.scope
    pres = (hidden_preacts(spec, P, sc + "/model", batch["obs"], layer_norm) +
            hidden_preacts(spec, P, sc + "/model", batch["next_obs"], layer_norm) +
            hidden_preacts(spec, P, sc + "/target_q_func/model", batch["next_obs"], layer_norm))
    lo = min(float(np.abs(p).min()) for p in pres)
    hi = max(float(np.abs(p).max()) for p in pres)
    return lo / hi


class Ref32(ql.QRef64):
    """The restatement evaluated in float32 (forward, backward; clip + Adam on float32-rounded values): the float32-faithful
    step of the layer-normalised case, which oracle/dqn.py cannot express."""

    def _tensors(self, grad=False):
        T = OrderedDict()
        for k, v in self.P64.items():
            T[k] = torch.from_numpy(v.astype(np.float32))
            if grad and k in self.train_names:
                T[k].requires_grad_(True)
        return T

    def q_values(self, obs):
        return ql.forward64(self.spec, self._tensors(), "%s/model" % self.spec.scope,
                            torch.from_numpy(np.asarray(obs, np.float32)), layer_norm=self.layer_norm).numpy()

    def grads(self, batch, weights):
        spec, T = self.spec, self._tensors(grad=True)
        b = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in batch.items()}
        w = torch.from_numpy(np.asarray(weights, np.float32))
        pre = "%s/model" % spec.scope
        q = ql.forward64(spec, T, pre, b["obs"], spec.trunk_scale, self.layer_norm)
        q_sel = torch.gather(q, 2, b["act"].long()[:, :, None]).squeeze(2)
        with torch.no_grad():
            q1 = ql.forward64(spec, T, pre, b["next_obs"], layer_norm=self.layer_norm)
            q2 = ql.forward64(spec, T, "%s/target_q_func/model" % spec.scope, b["next_obs"], layer_norm=self.layer_norm)
            sel = (q1 if spec.double_q else q2).argmax(dim=2)
            y = b["rew"] + spec.gamma * (1.0 - b["done"]) * torch.gather(q2, 2, sel[:, :, None]).squeeze(2).mean(dim=1)
        td = q_sel - y[:, None]
        err = torch.where(td.abs() < 1.0, 0.5 * td ** 2, td.abs() - 0.5) if spec.huber else td ** 2
        loss = torch.mean(w * (err.sum(dim=1) if (spec.algo == "bdq" and spec.loss_sum_branches) else err.mean(dim=1)))
        gs = torch.autograd.grad(loss, [T[n] for n in self.train_names])
        return {"loss": float(loss.detach()), "td": td.detach().numpy(), "priority": td.detach().abs().sum(dim=1).numpy(),
                "grads": {n: g.numpy().copy() for n, g in zip(self.train_names, gs)}}

    def step(self, batch, weights):
        out = super().step(batch, weights)
        for d in (self.P64, self.m, self.v):
            for n in d:
                d[n] = d[n].astype(np.float32).astype(np.float64)
        return out


# --------------------------------------------------------------------------------------------------- cases
def make_wide_case(name, **over):
    a = dict(WIDE_CASES[name] if name in WIDE_CASES else EDGE)
    a.update(over)
    seed, inputs = a.pop("seed"), a.pop("inputs")
    ln, per = bool(a.pop("layer_norm", False)), bool(a.pop("per", False))
    case = qu.make_q_case(seed=seed, n_steps=N_STEPS, uniform=True, **a)
    spec, tr = case["spec"], case["tr"]
    rng = np.random.default_rng(7000 + seed)
    shape = tr["obs"].shape
    if inputs == "pixels":
        tr["obs"], tr["next_obs"] = (rng.integers(0, 256, shape).astype(np.float32) for _ in range(2))
        tr["rew"] = rng.normal(0.0, 2.0, shape[0]).astype(np.float32)
    else:
        tr["obs"], tr["next_obs"] = (rng.normal(0.0, 1.0, shape).astype(np.float32) for _ in range(2))
        tr["rew"] = rng.normal(0.0, 0.05, shape[0]).astype(np.float32)
    P = ql.init_ln_params(spec, seed, ln)
    rows = np.concatenate([tr["obs"], tr["next_obs"]])
    for prefix in (spec.scope + "/model", spec.scope + "/target_q_func/model"):
        hidden_preacts(spec, P, prefix, rows, ln, calibrate=rng)
    if inputs == "normal":
        for n in P:
            if n.endswith("weights:0") and ql._is_out(spec, n):
                P[n] = (P[n] * np.float32(0.002)).astype(np.float32)
    c = case["cfg"]
    c.q_layer_norm = 1 if ln else 0
    if per:
        c.q_per, c.q_per_alpha, c.q_per_eps, c.q_per_alpha64 = 1, 0.6, 1e-6, 0.6
    case.update(params=P, layer_norm=ln, inputs=inputs, name=name)
    return case


def clip_scales(G, clip):
    return {n: clip / max(float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2))), clip) for n, g in G.items()}


def clip_rel(n):
    """Relative error bound of the engine's clip scale on a variable of n floats: a float32 sum of squares (terms >= 0) taken
    tile by tile and then over the tiles errs by at most (TILE + tiles) 2^-24, halved by the square root; two more roundings
    for the quotient and the product."""
    return (0.5 * (TILE + n // TILE + 1) + 2) * 2.0 ** -24


def reference_run(case):
    """The float64 trajectory: per-step outputs (with the margin of that update and its clip scales), the reference after the
    updates.  The target copy follows update 1, as in q_parity_util.run_and_compare."""
    spec = case["spec"]
    ref = ql.QRef64(spec, case["params"], case["layer_norm"])
    steps = []
    for s in range(case["n_steps"]):
        batch = ql.batch_of(case, s)
        m = margin(spec, ref.P64, batch, case["layer_norm"])
        out = ref.step(batch, case["weights"][s])
        out["margin"], out["scales"] = m, clip_scales(out["grads"], spec.grad_clip)
        steps.append(out)
        if s == 1:
            ref.update_target()
    return steps, ref


def float32_run(case):
    """The float32-faithful trajectory on the same inputs (oracle/dqn.py; layer norm: Ref32)."""
    spec = case["spec"]
    o = Ref32(spec, case["params"], True) if case["layer_norm"] else od.QOracle(spec, case["params"])
    steps = []
    for s in range(case["n_steps"]):
        steps.append(o.step(ql.batch_of(case, s), case["weights"][s]) if case["layer_norm"]
                     else o.step(qu._batch(case, s), case["weights"][s]))
        if s == 1:
            o.update_target()
    return steps, o


def assert_reference_conditions(case, steps):
    """On the reference alone, before anything is compared."""
    for s, out in enumerate(steps):
        assert out["margin"] > MARGIN_REL, "%s step %d: a hidden pre-activation lies %.2e x max from zero" % (case["name"], s, out["margin"])
        sc = out["scales"]
        big = [n for n, g in out["grads"].items() if g.size > WIDE_MIN]
        assert big
        if case["inputs"] == "pixels":
            assert all(sc[n] < 1.0 for n in big), (s, {n: sc[n] for n in big})
        else:
            assert all(v == 1.0 for v in sc.values()), (s, {n: v for n, v in sc.items() if v != 1.0})


def act_rows(case, n):
    rng = np.random.default_rng(900 + n)
    shape = (n, case["spec"].obs_dim)
    return (rng.integers(0, 256, shape) if case["inputs"] == "pixels" else rng.normal(0.0, 1.0, shape)).astype(np.float32)


def act_gap_ok(case, n):
    q = ql.QRef64(case["spec"], case["params"], case["layer_norm"]).q_values(act_rows(case, n))
    top = np.sort(q, axis=2)[:, :, -2:]
    return bool(((top[:, :, 1] - top[:, :, 0]) > ACT_GAP).all())


def find_seed(name, tries=50):
    """(development aid) the first seed of a case for which assert_reference_conditions and the act rows' gap hold"""
    for seed in range(tries):
        case = make_wide_case(name, seed=seed)
        steps, _ = reference_run(case)
        try:
            assert_reference_conditions(case, steps)
        except AssertionError:
            continue
        if all(act_gap_ok(case, n) for n in ACT_NS):
            return seed
    return None


# --------------------------------------------------------------------------------------------------- comparisons
_REF_CACHE = {}


def references(name):
    """(case, float64 steps, float64 end, float32 steps, float32 end), computed once per case and left unchanged"""
    if name not in _REF_CACHE:
        case = make_wide_case(name)
        s64, r64 = reference_run(case)
        s32, r32 = float32_run(case)
        _REF_CACHE[name] = (case, s64, r64, s32, r32)
    return _REF_CACHE[name]


def _dmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _within(got, ref, f32, atol, rtol, what, fig):
    """|got - ref| <= atol + rtol |ref| + 4 d_ref, d_ref = max |f32 - ref| of this quantity"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d_ref = _dmax(f32, ref)
    d = np.abs(got - ref)
    fig.append((what, d_ref, float(d.max())))
    print("%-34s d_ref %.3e   engine %.3e   (max |ref| %.3e)" % (what, d_ref, d.max(), np.abs(ref).max()))
    excess = d - (atol + rtol * np.abs(ref) + 4.0 * d_ref)
    assert excess.max() <= 0, "%s: max excess %.3e (max |d| %.3e, d_ref %.3e, max |ref| %.3e)" % (
        what, excess.max(), d.max(), d_ref, np.abs(ref).max())


def run_and_compare_wide(name, backend=None, lib_path=None):
    """q_parity_util.run_and_compare against the float64 reference with the wide yardstick; returns the figures
    [(quantity, d_ref, engine deviation)].  Also: the bucket holds the clipped gradient after the apply."""
    case, s64, r64, s32, r32 = references(name)
    assert_reference_conditions(case, s64)
    spec, fig = case["spec"], []
    print("%s: margins %s" % (name, ["%.2e" % o["margin"] for o in s64]))
    ref0 = ql.QRef64(spec, case["params"], case["layer_norm"])
    f0 = Ref32(spec, case["params"], True) if case["layer_norm"] else od.QOracle(spec, case["params"])
    eng = ql.engine_setup(case, backend, lib_path)
    try:
        obs4 = case["tr"]["obs"][:3]
        _within(eng.q_values(obs4), ref0.q_values(obs4), f0.q_values(obs4), 2e-5, 2e-4, "Q-values (act path)", fig)
        for s in range(case["n_steps"]):
            ref, f32 = s64[s], s32[s]
            eng.compute_grads(case["idx"][s:s + 1], case["weights"][s:s + 1])
            _within(eng.td_errors(), ref["td"], f32["td"], 3e-5, 2e-4, "td step %d" % s, fig)
            _within(eng.priorities(), ref["priority"], f32["priority"], 1e-4, 2e-4, "priority step %d" % s, fig)
            G = eng.get_gradients()
            if s == 0:
                for n, g in ref["grads"].items():
                    _within(G[n], g, f32["grads"][n], pu.GRAD_REL * max(np.abs(g).max(), 1e-12) + 1e-9, 0.0, "grad " + n.split("model/")[1], fig)
                _within(eng.metrics()["policy_loss"], ref["loss"], f32["loss"], 1e-6, 1e-4, "loss", fig)
            eng.apply_grads(1.0)
            # the bucket holds the clipped gradient: the engine's own sums through float64 clip_by_norm
            Gc, sc = eng.get_gradients(), clip_scales({n: G[n] for n in ref["grads"]}, spec.grad_clip)
            for n in ref["grads"]:
                if sc[n] == 1.0 and ref["scales"][n] == 1.0:
                    assert np.array_equal(Gc[n], G[n]), "bucket %s: scale 1 changed the gradient" % n
                else:
                    # float32 sum of squares, terms >= 0, taken tile by tile and then over the tiles: relative error at most
                    # (TILE + tiles) 2^-24, halved by the square root; two more roundings for the quotient and the product
                    rel = clip_rel(G[n].size)
                    want = np.asarray(G[n], np.float64) * sc[n]
                    assert _dmax(Gc[n], want) <= rel * np.abs(want).max(), "bucket %s: max |d| %.3e" % (n, _dmax(Gc[n], want))
                    assert abs(np.sqrt(np.sum(np.asarray(Gc[n], np.float64) ** 2)) - spec.grad_clip) <= rel * spec.grad_clip, n
            if s == 1:
                eng.update_target()
        P = eng.get_parameters()
        lr, n_steps = spec.lr, case["n_steps"]
        worst = (0.0, 0.0, "")
        for n, ref in r64.P64.items():
            d = np.abs(np.asarray(P[n], np.float64) - ref)
            dr = np.abs(np.asarray(r32.P[n], np.float64) - ref)
            worst = max(worst, (float(d.max()), float(dr.max()), n))
            assert d.max() <= 0.3 * lr * n_steps + 1e-7 + 4 * dr.max(), "param %s: max |d| %.3e (d_ref %.3e, lr %.1e)" % (n, d.max(), dr.max(), lr)
            assert d.mean() <= 0.02 * lr * n_steps + 1e-9 + 4 * dr.mean(), "param %s: mean |d| %.3e (d_ref %.3e)" % (n, d.mean(), dr.mean())
        fig.append(("parameters after %d updates" % n_steps, worst[1], worst[0]))
        print("%-34s d_ref %.3e   engine %.3e   (%s)" % ("parameters (worst tensor)", worst[1], worst[0], worst[2]))
        # the hard copy happened after update 1 only (kernels; a bias of magnitude 1e3 does not move by a step of 1e-6)
        assert all(not np.array_equal(P[n], P[n.replace("/target_q_func", "")]) for n in P
                   if "/target_q_func/" in n and n.endswith("weights:0"))
    finally:
        eng.close()
    return fig


def act_check(name, n, backend=None, lib_path=None):
    """grl_act(GRL_ACT_GREEDY) on n rows == the arg-max of the reference; every (row, branch) has a top-two gap above ACT_GAP in
    float64 (asserted first, on the reference alone)."""
    case = references(name)[0]
    obs = act_rows(case, n)
    q = ql.QRef64(case["spec"], case["params"], case["layer_norm"]).q_values(obs)
    top = np.sort(q, axis=2)[:, :, -2:]
    assert ((top[:, :, 1] - top[:, :, 0]) > ACT_GAP).all()
    eng = ql.engine_setup(case, backend, lib_path, act_batch=n)
    try:
        bins = eng.act_bins(obs)
        assert np.array_equal(bins, q.argmax(axis=2))
        assert np.array_equal(eng.act_bins(obs[:1]), bins[:1]) and np.array_equal(eng.act_bins(obs), bins)
        assert np.array_equal(eng.q_values(obs).argmax(axis=2), bins)
    finally:
        case["cfg"].act_batch = 4
        eng.close()


def _end_state(eng):
    return (eng.get_parameters(), eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy(), eng.sampled_indices(), eng.metrics(),
            eng.fetch("grads").copy())


def _same(a, b, what):
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), (what, k)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what
    assert np.array_equal(a[3], b[3]) and a[4] == b[4], what
    assert np.array_equal(a[5], b[5]), what + ": gradient bucket"


def multi_update_check(name, backend_factory, lib_path=None, n=4):
    """Device RNG (prioritised for the `per` case): ONE call of n updates == n calls of one == a second run from the same state,
    bit for bit -- parameters, moments, drawn indices, metrics and the bucket (no order dependence in the partial sums)."""
    case = references(name)[0]
    per = bool(case["cfg"].q_per)

    def run(split):
        eng = ql.engine_setup(case, backend_factory(), lib_path)
        for k in split:
            eng.train_per(k, 0.7) if per else eng.train_device(k)
        out = _end_state(eng)
        eng.close()
        return out
    ref = run([1] * n)
    _same(ref, run([1] * n), "second run from the same state")
    _same(ref, run([n]), "one call of n updates")
    _same(ref, run([1, n - 1]), "1 + (n - 1)")
    assert any(not np.array_equal(ref[0][k], case["params"][k]) for k in ref[0] if k.endswith("weights:0") and "/target_q_func/" not in k)


def checkpoint_check(name, backend_factory, path, lib_path=None, n=2):
    """n updates, checkpoint, a NEW handle, n more == 2 n updates on one handle, bit for bit."""
    import checkpoint_util as cu
    case = references(name)[0]

    class Run:
        def bare(self):
            return ql.QEngine(case["cfg"], backend=backend_factory(), lib_path=lib_path)

        def prepared(self, wrap):
            return ql.engine_setup(case, backend_factory(), lib_path)

        def train(self, eng, k):
            eng.train_device(k)
    a, b, _ = cu.continuation(Run(), path, n, wrap=False)
    try:
        cu.assert_same_training_state(a, b, name)
        _same(_end_state(a), _end_state(b), "continued from the checkpoint")
    finally:
        a.close()
        b.close()


def edge_plan(obs_dim, read_plan, backend=None, lib_path=None):
    """The plan dump of the EDGE network at obs_dim; one update runs (the plan is exercised, not only printed)."""
    case = make_wide_case("edge", obs_dim=obs_dim)
    eng = ql.engine_setup(case, backend, lib_path)
    try:
        plan = read_plan()
        eng.train(1, case["idx"][:1], case["weights"][:1])
        assert all(np.isfinite(v).all() for v in eng.get_parameters().values())
    finally:
        eng.close()
    return plan


def wide_line(plan):
    """the `grl plan: q_wide` line of a dump (a handle plans twice -- sizing pass, then the real one -- and says the same both
    times), None when there is none"""
    lines = set(ln for ln in plan.splitlines() if ln.startswith("grl plan: q_wide"))
    assert len(lines) <= 1, lines
    return lines.pop() if lines else None
