"""The references of tests/sac_edge_util.py on their own, without an engine: the oracle's dtype argument (float32 default
bit-identical to the oracle before it had one, float64 the same graph), the float64 closed form of the policy head's elements
against float64 autograd of oracle.sac.actor_fwd, and `assert_regime` on every case the device file trains on."""
import hashlib
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import parity_util as pu
import sac_edge_util as se
from oracle import sac as osac

PIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sac_oracle_float32_pin.npz")
PIN_CASE = dict(extractor="mlp", B=17, n_replay=64, layers=(96, 72), obs_dim=29, act_dim=7)      # test_gpu_parity.py: mlp_layers_96_72


def oracle_pin(mod):
    """Two updates of PIN_CASE with the SacOracle of module `mod` (default arguments): first-step tensors, losses and gradients,
    final parameters and moments.  tests/golden/sac_oracle_float32_pin.npz holds this for oracle/sac.py as it was before
    SacOracle had a dtype argument (written once with that file as `mod`)."""
    case = pu.make_case(n_steps=2, **PIN_CASE)
    orc = mod.SacOracle(case["spec"], case["params"])
    out = OrderedDict()
    for s in range(2):
        raw = {k: case["tr"][k][case["idx"][s]] for k in ("obs", "act", "rew", "next_obs", "done")}
        d = orc.step(mod.prepare_batch(case["spec"], raw, case["stats"]), case["eps"][s])
        for k in ("mu", "log_std", "pi", "logp", "v", "qf1", "qf1_pi", "policy_loss", "value_loss", "qf1_loss", "ent_loss", "ent_coef"):
            out["s%d/%s" % (s, k)] = np.asarray(d[k])
        for n, g in d["grads"].items():
            out["s%d/grad/%s" % (s, n)] = g
    for n, v in orc.P.items():
        out["P/" + n] = v
    for i, st in enumerate(orc.opt):
        for n in st["m"]:
            out["m%d/%s" % (i, n)], out["v%d/%s" % (i, n)] = st["m"][n], st["v"][n]
    for k, v in out.items():          # tensors of more than 512 elements as the SHA-256 of their bytes
        assert v.dtype == np.float32, k
        out[k] = v if v.size <= 512 else np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), np.uint8)
    return out


def test_the_default_dtype_keeps_the_oracles_bits():
    pin = np.load(PIN)
    now = oracle_pin(osac)
    assert sorted(now) == sorted(pin.files)
    for k, v in now.items():
        assert v.dtype == pin[k].dtype and v.shape == pin[k].shape, k
        assert v.tobytes() == pin[k].tobytes(), k


def test_float64_is_the_same_graph():
    case = se.make_case("mlp_96_72", "clip")
    out = {}
    for dt in (torch.float32, torch.float64):
        orc = osac.SacOracle(case["spec"], case["params"], dtype=dt)
        out[dt] = orc.step(se.batch_of(case, 0, dt), case["eps"][0])
        assert all(v.dtype == np.float32 for v in orc.P.values())
    a, b = out[torch.float32], out[torch.float64]
    assert b["logp"].dtype == np.float64 and a["logp"].dtype == np.float32
    assert all(g.dtype == np.float64 for g in b["grads"].values())
    for k in ("mu", "pi", "v", "qf1", "qf2", "qf1_pi"):
        pu.close(a[k], b[k], what=k)
    for n in b["grads"]:
        pu.close_rel_max(a["grads"][n], b["grads"][n], what=n)
    assert float(b["ent_loss"]) != 0.0


# --------------------------------------------------------------------------------------------------- the closed form
def autograd_elements(mu, ls_raw, eps, da, alpha):
    """logp, t, dmu, dls of L = mean(alpha logp) + sum(da pi) by float64 autograd through oracle.sac.actor_fwd: a policy without
    hidden layers on the rows of an identity, so that the two output kernels ARE mu and the raw log-std."""
    B, A = mu.shape
    spec = osac.SacSpec(extractor="mlp", obs_dim=B, act_dim=A, layers=[])
    T = {"model/pi/dense/kernel:0": torch.tensor(mu, dtype=torch.float64, requires_grad=True),
         "model/pi/dense_1/kernel:0": torch.tensor(ls_raw, dtype=torch.float64, requires_grad=True),
         "model/pi/dense/bias:0": torch.zeros(A, dtype=torch.float64), "model/pi/dense_1/bias:0": torch.zeros(A, dtype=torch.float64)}
    a = osac.actor_fwd(spec, T, torch.eye(B, dtype=torch.float64), torch.tensor(eps, dtype=torch.float64))
    assert torch.equal(a["mu"], T["model/pi/dense/kernel:0"])
    loss = torch.mean(alpha * a["logp"]) + torch.sum(torch.tensor(da, dtype=torch.float64) * a["pi"])
    dmu, dls = torch.autograd.grad(loss, [T["model/pi/dense/kernel:0"], T["model/pi/dense_1/kernel:0"]])
    return a["logp"].detach().numpy(), a["pi"].detach().numpy(), dmu.numpy(), dls.numpy()


def _hold(got, ref, mag, what):
    d = np.abs(got - ref)
    assert (d <= 1e-10 * mag).all(), "%s: relative %.3e" % (what, (d / np.maximum(mag, 1e-300)).max())


def check_closed_form(mu, ls_raw, eps, da, alpha=0.2):
    B = mu.shape[0]
    logp, t, dmu, dls = autograd_elements(mu, ls_raw, eps, da, alpha)
    cf = se.closed_form(mu, ls_raw, eps, t, da, alpha, B)
    _hold(cf["logp"], logp, np.abs(logp), "logp")
    # relative to the larger of the value and its addends: the two addends of an element may cancel
    _hold(cf["dmu"], dmu, np.maximum(np.abs(dmu), np.abs(cf["dmu_q"]) + np.abs(cf["dmu_lp"])), "dmu")
    _hold(cf["dls"], dls, np.maximum(np.abs(dls), np.abs(cf["dls_u"]) + np.abs(cf["dls_g"])), "dls")
    return cf, t, dmu, dls


@pytest.mark.parametrize("regime", ["clip", "saturated", "near_saturated", "small_sd", "combined"])
def test_closed_form_against_float64_autograd(regime):
    """On the head inputs of the regime's mlp (96, 72) case (float64 mu and raw log-std of its first minibatch, its noise)."""
    case = se.make_case("mlp_96_72", regime)
    mu, ls = se.head_inputs64(case, 0)
    eps = case["eps"][0].astype(np.float64)
    da = np.random.default_rng(1).normal(0.0, 0.3, mu.shape)
    cf, t, dmu, dls = check_closed_form(mu, ls, eps, da)
    if regime == "saturated":
        sat = np.abs(cf["u"]) >= 20.0
        assert sat.any() and (np.abs(t[sat]) == 1.0).all() and (dmu[sat] == 0.0).all() and np.isfinite(cf["logp"]).all()
    if regime in ("clip", "combined"):
        assert (dls[:, 2:4] == 0.0).all() and (cf["dls"][:, 2:4] == 0.0).all() and (dls[:, :2] != 0.0).all()
        assert (ls[:, 0] == 2.0).all() and (ls[:, 1] == -20.0).all()


def test_closed_form_at_and_beyond_the_clip_boundaries():
    """Raw log-std exactly 2.0 and -20.0: the gradient passes (TF's maximum / minimum gradients and torch.clamp are inclusive at
    equality); one float64 step outside and far outside: exactly 0."""
    ls = np.array([[2.0, -20.0, np.nextafter(2.0, 3.0), np.nextafter(-20.0, -21.0), 2.5, -25.0, 7.0, -300.0, np.nextafter(2.0, 0.0), np.nextafter(-20.0, 0.0)]])
    ls = np.repeat(ls, 4, 0)
    rng = np.random.default_rng(2)
    mu, eps, da = rng.normal(0, 0.5, ls.shape), rng.normal(0, 0.05, ls.shape), rng.normal(0, 0.3, ls.shape)
    cf, t, dmu, dls = check_closed_form(mu, ls, eps, da)
    passes = [0, 1, 8, 9]
    blocked = [2, 3, 4, 5, 6, 7]
    assert (dls[:, passes] != 0.0).all() and (cf["dls"][:, passes] != 0.0).all()
    assert (dls[:, blocked] == 0.0).all() and (cf["dls"][:, blocked] == 0.0).all()
    assert (dmu != 0.0).all()                      # the mask is on the log-std path alone


def test_the_bounds_contain_a_float32_model_of_the_formula():
    """numpy float32 arithmetic of the formula, fed its own float32 tanh, stays inside the derived bounds in every regime (and
    below a quarter of the logp bound's first term)."""
    f = np.float32
    for regime in ("clip", "saturated", "near_saturated", "small_sd"):
        case = se.make_case("mlp_96_72", regime)
        mu64, ls64 = se.head_inputs64(case, 0)
        mu, lr, ep = mu64.astype(f), ls64.astype(f), case["eps"][0]
        da = np.random.default_rng(1).normal(0.0, 0.3, mu.shape).astype(f)
        B = mu.shape[0]
        ls = np.clip(lr, f(-20), f(2)); sd = np.exp(ls); u = mu + ep * sd
        t = np.tanh(u.astype(np.float64)).astype(f)
        z = (u - mu) / (sd + f(1e-6)); omt = f(1) - t * t
        logp = (f(-0.5) * (z * z + f(2) * ls + f(1.8378770664093453)) - np.log(omt + f(1e-6))).sum(1, dtype=f)
        aob = np.exp(se.LOG_ENT_COEF) / f(B)
        dmu = da * omt + aob * (f(2) * t * omt / (omt + f(1e-6)))
        den = sd + f(1e-6)
        dls = dmu * sd * ep + aob * (-((sd * ep / den) * (ep * sd * f(1e-6) / (den * den)) + f(1)))
        dls = np.where((lr < f(-20)) | (lr > f(2)), f(0), dls)
        cf = se.closed_form(mu, lr, ep, t, da, float(np.exp(np.float64(se.LOG_ENT_COEF))), B)
        bd = se.element_bounds(cf, t, da, ep)
        first = (2.0 ** -23 / (cf["omt"] + se.EPS)).sum(1)
        z_part = (np.abs(cf["z"]) * (se.ulp32(cf["u"]) / (cf["sd"] + se.EPS)) + 0.5 * (se.ulp32(cf["u"]) / (cf["sd"] + se.EPS)) ** 2).sum(1)
        d_logp = np.abs(logp - cf["logp"])
        assert (d_logp <= bd["logp"]).all(), regime
        assert (np.maximum(d_logp - z_part - 1e-5 * (1 + np.abs(cf["logp"])), 0) <= 0.25 * first).all(), regime
        assert (np.abs(dmu - cf["dmu"]) <= bd["dmu"]).all(), regime
        assert (np.abs(dls - cf["dls"]) <= bd["dls"]).all(), regime


# --------------------------------------------------------------------------------------------------- the regimes
@pytest.mark.parametrize("shape,regime", se.TRAIN_CASES, ids=lambda v: str(v))
def test_every_case_is_what_its_regime_claims(shape, regime):
    se.assert_regime(se.make_case(shape, regime))
