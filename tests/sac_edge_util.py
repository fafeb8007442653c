"""The squashed-Gaussian policy head of SAC at its numeric edges: the log-std clip and its gradient mask, saturated tanh, the
`+ EPS` guards, sd ~ EPS, and an entropy coefficient that is not 1.  Shared by tests/test_gpu_sac_policy_edges.py (device),
tests/test_hostemu_sac_policy_edges.py (emulation build) and tests/test_sac_edge_host.py (the references on their own).

Every other SAC parity case starts from oracle.sac.init_params (zero biases, log_ent_coef = 0): |mu|, |log_std| < 2, tanh far from
+-1, alpha = 1, log_alpha = 0.  A REGIME here moves the biases of `dense` / `dense_1`, scales the policy noise per column and
sets log_ent_coef = log(0.2):

  clip            columns (A = 5 uses the first five)
                  0  dense_1 kernel column 0, bias  2.0   on the upper boundary in every row: the gradient passes
                  1  dense_1 kernel column 0, bias -20.0  on the lower boundary in every row: the gradient passes
                  2  kernel column * 0.2,     bias  2.5   above the range in every row: dls == 0, kernel / bias gradient == 0
                  3  kernel kept,             bias -25.0  below the range in every row: the same
                  4  kernel kept,             bias  2.0 - m   rows on both sides of the upper boundary
                  5  untouched
                  6  kernel kept,             bias -20.0 - m  rows on both sides of the lower boundary
                  (m: the midpoint of the column's two middle rows without the bias, so that B // 2 rows lie at or below the
                  boundary whatever the extractor feeds the head; behind the CNN all rows of a column fall on one side of a fixed 2.0)
                  noise of columns 0, 2, 4, 5 is chosen per element so that u = mu + eps sd is uniform in +-1.49
  saturated       mu bias +30 / -30 on columns 0, 1, 3, 5: |u| >= 15, tanhf(u) = +-1 and 1 - t^2 = 0 exactly in float32;
                  the other columns as column 5 above
  near_saturated  mu bias 3 .. 6 (alternating sign), log_std bias -1 .. -2: 1 - t^2 between 1e-7 and 1e-2
  small_sd        log_std bias -12 / -13.8 (sd ~ EPS) / -16, mu bias 1
  combined        the log-std columns of `clip` with mu bias +-30 on columns 0, 3, 6 (bit checks only)

`assert_regime` checks ON THE FLOAT64 REFERENCE ALONE, before anything is compared, that a case is what its regime claims
(conditions, not tolerances); SEEDS holds the first seed of each (shape, regime) at which it does (`find_seed`).

REFERENCES.  (1) oracle.sac.SacOracle(dtype=torch.float64): the oracle's own graph on widened float32 inputs.  The float32
oracle cannot referee here: at sd ~ EPS its autograd differentiates through u - mu AFTER u = mu + eps sd was rounded, which
loses 2 % of z = (u - mu) / (sd + EPS) where mu ~ 1, while the engine's analytic backward is right to 1e-7.  (2) `closed_form`:
the head's elements restated in float64 from the published formula, not from the kernels:
    ls = clip(ls_raw, -20, 2), sd = exp(ls), u = mu + eps sd, t = tanh(u), z = (u - mu) / (sd + EPS) = eps sd / (sd + EPS)
    logp = sum_j -0.5 (z^2 + 2 ls + log 2 pi) - log(1 - t^2 + EPS)
  With L = (alpha / B) sum_b logp_b + sum da * t (da = d policy_loss / d pi, what the qf1 head's backward hands over):
    dL/du   = da (1 - t^2) + (alpha / B) 2 t (1 - t^2) / (1 - t^2 + EPS)        (d/du of -log(1 - t^2 + EPS))
    dL/dmu  = dL/du                                     (the Gaussian term has no mu-gradient: u - mu = eps sd)
    dz/dls  = eps sd EPS / (sd + EPS)^2
    dL/dls  = dL/du eps sd - (alpha / B)(z dz/dls + 1)  where -20 <= ls_raw <= 2 (inclusive: TF's maximum / minimum gradients
              and torch.clamp pass the gradient at equality), exactly 0 outside
  tests/test_sac_edge_host.py holds it to 1e-10 against float64 autograd of oracle.sac.actor_fwd on every regime.

LEVEL A (`check_elements`, every regime): the engine's stored elements against `closed_form` evaluated with the engine's own
float32 mu, log_std, da_pi and -- except for pi itself -- its own pi, so the rounding of tanhf drops out and one nearly
saturated element cannot poison a whole tensor.  With ulp(x) the float32 spacing at x and e = 2^-24:
  pi    |pi - tanh64(u)| <= K_ULP ulp(t) + (1 - t^2)(ulp(u) + |eps sd| 2^-23): K_ULP for tanhf itself, the rest for the one or two
        roundings of u in front of it (<= ulp(u) together) and the <= 1 ulp of expf in sd, each carried through tanh' = 1 - t^2.
        K_ULP = 1: MEASURED worst excess on the MI355X over all cases of tests/test_gpu_sac_policy_edges.py 0.494 ulp
        (reference float64 tanh); twice that, rounded up to an integer, is 1.  (glibc's tanhf on the emulation build: 0.930.)
  logp  per row  sum_j [ 2^-23 / (1 - t_j^2 + EPS) + |z_j| dz_j + dz_j^2 / 2 ] + 1e-5 (1 + |ref|),  dz_j = ulp(u_j) / (sd_j + EPS):
        1 - t t carries an absolute error of <= 2^-23 (t t: e, the subtraction: e, the sum with EPS: within that again at
        1 - t^2 <= 1), which the logarithm divides by its argument; the kernel forms z from the ROUNDED u, an error dz in z
        that -0.5 z^2 turns into |z| dz + dz^2 / 2; 1e-5 (1 + |ref|) for expf / logf and the sum over A.
  dmu   with d_omt = 2^-23 the same absolute error of omt = 1 - t^2, r = omt / (omt + EPS), dr/d omt = EPS / (omt + EPS)^2:
        |da| d_omt + (alpha / B) 2 |t| EPS / (omt + EPS)^2 d_omt + 8 e (|da omt| + |(alpha / B) 2 t r|)
        (8 roundings at most on either addend: the products, omt + EPS, the division, expf(log_alpha) to 1 ulp = 2 e, the
        division by B, the final sum).
  dls   |eps sd| bound(dmu) + 32 e (|dL/du eps sd| + |(alpha / B)(z dz/dls + 1)|): sd = expf(ls) to 1 ulp (2 e) enters z
        (7 e with its product, sum and quotient), dz/dls (12 e), their product (20 e), the + 1, alpha / B (3 e) and its product
        -- 26 e on the second addend, 4 e on the first, one for the sum: 32 e bounds them all.
  exact outside the clip: dls == +0.0 bitwise; saturated (|u| >= 15): pi == +-1, dmu == 0, logp finite.
  hand-over: gradient of model/pi/dense/bias == sum_b dmu, of model/pi/dense_1/bias == sum_b dls (float64 sums of the engine's
  elements, within 1e-5 of sum_b |element|: a float32 sum of B values errs by up to (B - 1) e of the summands' magnitudes, not
  of a result they may cancel in -- the untouched column of `clip` at (48, 40) cancels to 2.7e-4 from summands of 1e-2 and
  sits 1.03e-5 of its own value off); loss scalars and the gradient of log_ent_coef recomputed in float64 from the engine's own
  fetched logp, v, qf*, rew, done (1e-5 relative); ent_coef_loss must be nonzero on the reference.

LEVEL B (`check_end_to_end`; clip, saturated, small_sd): mu, qf*, v (parity_util FWD_ATOL / FWD_RTOL) and every policy and
value-function gradient (parity_util.GRAD_REL through close_rel_max) against the float64 oracle graph, then a second update
and parity_util.compare_params.  In small_sd the value group is left out: it consumes logp (v_backup = min q - alpha logp), and
logp is ill-conditioned there -- the forward's z comes from the rounded u, 1.5e-2 absolute in float32 for the engine and the
float32 oracle alike.  near_saturated has no level B: a few elements with 1 - t^2 ~ 1e-6 move whole tensors by percent per
ulp of tanhf.
"""
import functools
from collections import OrderedDict

import numpy as np
import torch

import parity_util as pu
from grasp_rl import _capi
from oracle import sac as osac

EPS = osac.EPS
LOG2PI = float(np.log(2.0 * np.pi))
LOG_ENT_COEF = np.float32(np.log(0.2))
E = 2.0 ** -24                  # unit roundoff of float32
# tanhf against float64 tanh, in ulp of the result, beyond the rounding of u (see LEVEL A above).  Measured on the MI355X: worst
# 0.494 ulp over all cases -> 2 x 0.494 rounded up to an integer = 1; the emulation build (glibc tanhf) reaches 0.930.
K_ULP = 1
WORST = {"pi_ulp": 0.0}         # the worst excess this process has seen (printed by the tests, for the figure above)

FIT = "fit"                     # noise chosen per element so that u is uniform in +-U_FIT
U_FIT = 1.49
REGIMES = {
    "clip": dict(mu_bias=[0, 0, 0, 0, 0, 0, 0], ls_bias=[2.0, -20.0, 2.5, -25.0, 2.0, 0.0, -20.0],
                 ls_kernel=[0.0, 0.0, 0.2, 1.0, 1.0, 1.0, 1.0], eps=[FIT, 1.0, FIT, 1.0, FIT, FIT, 1.0], straddle=[4, 6]),
    "saturated": dict(mu_bias=[30.0, -30.0, 0, 30.0, 0, -30.0, 0], ls_bias=[0] * 7, ls_kernel=[1.0] * 7,
                      eps=[0.3, 0.3, FIT, 0.3, FIT, 0.3, FIT]),
    "near_saturated": dict(mu_bias=[3.0, -3.5, 4.0, -4.5, 5.0, -5.5, 6.0], ls_bias=[-1.0, -1.25, -1.5, -1.75, -2.0, -1.5, -1.0],
                           ls_kernel=[1.0] * 7, eps=[1.0] * 7),
    "small_sd": dict(mu_bias=[1.0] * 7, ls_bias=[-12.0, -13.8, -16.0, -13.8, -12.0, -16.0, -13.8], ls_kernel=[1.0] * 7, eps=[1.0] * 7),
    "combined": dict(mu_bias=[30.0, 0, 0, -30.0, 0, 0, 30.0], ls_bias=[2.0, -20.0, 2.5, -25.0, 2.0, 0.0, -20.0],
                     ls_kernel=[0.0, 0.0, 0.2, 1.0, 1.0, 1.0, 1.0], eps=[0.02, 1.0, 0.02, 1.0, 0.02, 0.3, 1.0], straddle=[4, 6]),
}
WELL_CONDITIONED = ("clip", "saturated", "small_sd")
STRADDLE_MARGIN = 1e-4          # no raw log-std of a straddling column this close to the boundary (float32 could take the other side)

SHAPES = {
    "mlp_96_72": dict(extractor="mlp", B=17, n_replay=64, layers=(96, 72), obs_dim=29, act_dim=7),     # two 16-row blocks, the second ragged; ragged A
    "mlp_48_40": dict(extractor="mlp", B=17, n_replay=64, layers=(48, 40), obs_dim=29, act_dim=7),     # the same on the one-launch matrix-core route
    "mlp_260": dict(extractor="mlp", B=5, n_replay=16, layers=(260,), obs_dim=29, act_dim=5),          # wider than HT_MAXW: per layer without a switch
    "augmented": dict(extractor="augmented", kind="depth", B=6, n_replay=24, act_dim=5),               # the staged CNN plan
    "mlp_b1": dict(extractor="mlp", B=1, n_replay=4, layers=(64, 64), obs_dim=101, act_dim=5),
    "act_64_64": dict(extractor="mlp", B=4, n_replay=20, layers=(64, 64), obs_dim=101, act_dim=5),
    "act_260": dict(extractor="mlp", B=4, n_replay=20, layers=(260,), obs_dim=101, act_dim=5),
}
# (shape, regime) -> the first seed at which assert_regime holds (find_seed); 0 where not listed
SEEDS = {}

# every case the device file trains on: tests/test_sac_edge_host.py runs assert_regime on each
TRAIN_CASES = ([("mlp_96_72", r) for r in ("clip", "saturated", "near_saturated", "small_sd")] +
               [("mlp_48_40", r) for r in ("clip", "saturated", "near_saturated", "small_sd")] +
               [(s, r) for s in ("mlp_260", "augmented") for r in ("clip", "saturated")] + [("mlp_b1", "saturated")])


# --------------------------------------------------------------------------------------------------- cases
def columns(regime, A):
    r = REGIMES[regime]
    return {k: ([j for j in v if j < A] if k == "straddle" else list(v[:A])) for k, v in r.items()}


def batch_of(case, s, dtype=torch.float32):
    tr, ii, nm = case["tr"], case["idx"][s], case["normalize"]
    raw = {k: tr[k][ii] for k in ("obs", "act", "rew", "next_obs", "done")}
    return osac.prepare_batch(case["spec"], raw, case["stats"] if nm else None, norm_obs=nm in (True, "obs"),
                              norm_reward=nm in (True, "reward"), dtype=dtype)


def head_inputs64(case, s=0):
    """mu and the RAW log-std of minibatch s at the case's parameters: the oracle's functions on float64 tensors."""
    spec = case["spec"]
    T = osac.SacOracle(spec, case["params"], dtype=torch.float64).tensors()
    with torch.no_grad():
        z = osac.mlp_fwd(spec, T, "model/pi", osac.extractor_fwd(spec, T, "model/pi", batch_of(case, s, torch.float64)["obs"]))
        return osac.dense(T, "model/pi", "dense", z).numpy(), osac.dense(T, "model/pi", "dense_1", z).numpy()


def apply_regime(params, regime, A):
    c = columns(regime, A)
    P = OrderedDict((n, np.array(v, np.float32)) for n, v in params.items())
    P["model/pi/dense/bias:0"] = np.asarray(c["mu_bias"], np.float32)
    P["model/pi/dense_1/bias:0"] = np.asarray(c["ls_bias"], np.float32)
    P["model/pi/dense_1/kernel:0"] = (P["model/pi/dense_1/kernel:0"] * np.asarray(c["ls_kernel"], np.float32)[None, :]).astype(np.float32)
    P["model/log_ent_coef:0"] = LOG_ENT_COEF.reshape(())
    return P


def make_case(shape, regime, n_steps=2, act_batch=4, seed=None):
    kw = SHAPES[shape]
    seed = SEEDS.get((shape, regime), 0) if seed is None else seed
    case = pu.make_case(n_steps=n_steps, seed=seed, **kw)
    if act_batch != 4:
        case["cfg"] = _capi.make_config("mlp", obs_dim=kw["obs_dim"], act_dim=kw["act_dim"], layers=kw["layers"], batch_size=kw["B"],
                                        replay_capacity=kw["n_replay"], normalize=True, act_batch=act_batch)
    A, B = kw["act_dim"], kw["B"]
    case.update(name="%s-%s" % (shape, regime), shape=shape, regime=regime, params=apply_regime(case["params"], regime, A))
    c = columns(regime, A)
    if B > 1:        # a straddling column's bias moves by the midpoint of its two middle rows: B // 2 rows at or below the boundary
        _, ls = head_inputs64(case, 0)
        for j in c.get("straddle", []):
            col = np.sort(ls[:, j] - c["ls_bias"][j])
            case["params"]["model/pi/dense_1/bias:0"][j] = np.float32(c["ls_bias"][j] - 0.5 * (col[B // 2 - 1] + col[B // 2]))
    rng = np.random.default_rng(seed + 11)
    scale = np.asarray([0.02 if e == FIT else e for e in c["eps"]], np.float32)
    eps = (rng.standard_normal((n_steps, B, A)) * scale).astype(np.float32)
    fit = [j for j in range(A) if c["eps"][j] == FIT]
    if fit:          # the compared (first) minibatch: u uniform in +-U_FIT on these columns
        mu, ls = head_inputs64(case, 0)
        sd = np.exp(np.clip(ls, osac.LOG_STD_MIN, osac.LOG_STD_MAX))
        target = rng.uniform(-U_FIT, U_FIT, (B, A))
        eps[0][:, fit] = ((target - mu) / sd)[:, fit].astype(np.float32)
    case["eps"] = eps
    return case


@functools.lru_cache(maxsize=None)
def case_with_reference(shape, regime, n_steps=2):
    """The case and its float64 run (per-step diagnostics, the oracle after n_steps updates): computed once per process, shared by
    every test that needs it, never modified."""
    case = make_case(shape, regime, n_steps)
    orc = osac.SacOracle(case["spec"], case["params"], dtype=torch.float64)
    out = []
    for s in range(n_steps):
        batch = batch_of(case, s, torch.float64)
        d = orc.step(batch, case["eps"][s])
        d["batch"] = batch
        out.append(d)
    case["ref64"], case["orc64"] = out, orc
    return case


def sech2(u):
    """1 - tanh(u)^2 without the cancellation"""
    return 1.0 / np.cosh(np.minimum(np.abs(u), 300.0)) ** 2


def assert_regime(case):
    """On the float64 reference alone: the case is what its regime claims (conditions, not tolerances)."""
    regime, B, A = case["regime"], case["B"], case["spec"].act_dim
    c = columns(regime, A)
    mu, ls = head_inputs64(case, 0)
    eps = case["eps"][0].astype(np.float64)
    u = mu + eps * np.exp(np.clip(ls, osac.LOG_STD_MIN, osac.LOG_STD_MAX))
    omt = sech2(u)
    name = case["name"]
    assert np.float32(case["params"]["model/log_ent_coef:0"]) == LOG_ENT_COEF != 0.0
    if regime in WELL_CONDITIONED:
        bad = ~((np.abs(u) >= 15.0) | (omt >= 1e-2))
        assert not bad.any(), "%s: %d elements are neither saturated nor well inside (|u| %s)" % (name, bad.sum(), np.abs(u)[bad])
    if regime == "clip":
        n = min(3, B // 2)
        for j, b in ((0, 2.0), (1, -20.0)):
            assert (ls[:, j] == b).all(), "%s: column %d is not on the boundary in every row" % (name, j)
        assert (ls[:, 2] > osac.LOG_STD_MAX).all() and (ls[:, 3] < osac.LOG_STD_MIN).all(), name + ": columns 2 / 3 are not outside in every row"
        assert (ls[:, 4] > 2.0).sum() >= n and (ls[:, 4] <= 2.0).sum() >= n, "%s: straddle column %s" % (name, ls[:, 4])
        assert (np.abs(ls[:, 4] - 2.0) > STRADDLE_MARGIN).all(), name
        if A > 6:
            assert (ls[:, 6] < -20.0).sum() >= n and (ls[:, 6] >= -20.0).sum() >= n and (np.abs(ls[:, 6] + 20.0) > STRADDLE_MARGIN).all(), name
        for j in (0, 2, 4):
            assert (np.abs(u[:, j]) <= 1.5).all(), "%s: high-sd column %d leaves |u| <= 1.5" % (name, j)
    if regime == "saturated":
        sat = [j for j in range(A) if c["mu_bias"][j] != 0]
        assert (np.abs(u[:, sat]) >= 15.0).all(), name
    if regime == "near_saturated":
        k = int(((omt >= 1e-7) & (omt <= 1e-3)).sum())
        assert 2 * k >= B, "%s: only %d elements with 1e-7 <= 1 - t^2 <= 1e-3" % (name, k)
        assert omt.min() < 1e-5 and omt.max() > 1e-3, name
    if regime == "small_sd":
        sd = np.exp(ls)
        assert (sd < 2e-5).all() and (sd > 1e-8).all() and ((sd > 0.5 * EPS) & (sd < 2 * EPS)).any(), name


def find_seed(shape, regime, tries=200):
    for seed in range(tries):
        try:
            assert_regime(make_case(shape, regime, seed=seed))
            return seed
        except AssertionError:
            pass
    raise AssertionError("no seed for %s / %s" % (shape, regime))


# --------------------------------------------------------------------------------------------------- the closed form
def closed_form(mu, ls_raw, eps, t, da, alpha, B):
    """The head's elements in float64 (module docstring).  Returns logp [B], its per-element terms, dmu, dls [B, A], the two
    addends of each (`*_q` through pi, `*_lp` / `*_g` through logp) and the intermediate quantities the bounds need."""
    mu, ls_raw, eps, t, da = (np.asarray(x, np.float64) for x in (mu, ls_raw, eps, t, da))
    ls = np.clip(ls_raw, osac.LOG_STD_MIN, osac.LOG_STD_MAX)
    sd = np.exp(ls)
    z = eps * sd / (sd + EPS)
    gauss = -0.5 * (z * z + 2.0 * ls + LOG2PI)
    omt = 1.0 - t * t
    squash = -np.log(omt + EPS)
    aob = alpha / B
    dmu_q = da * omt
    dmu_lp = aob * 2.0 * t * omt / (omt + EPS)
    dmu = dmu_q + dmu_lp
    dz = eps * sd * EPS / (sd + EPS) ** 2
    inside = (ls_raw >= osac.LOG_STD_MIN) & (ls_raw <= osac.LOG_STD_MAX)
    dls_u = dmu * eps * sd
    dls_g = -aob * (z * dz + 1.0)
    return dict(ls=ls, sd=sd, u=mu + eps * sd, z=z, omt=omt, gauss=gauss, squash=squash, logp=(gauss + squash).sum(1), aob=aob,
                dmu=dmu, dmu_q=dmu_q, dmu_lp=dmu_lp, inside=inside, dls=np.where(inside, dls_u + dls_g, 0.0),
                dls_u=np.where(inside, dls_u, 0.0), dls_g=np.where(inside, dls_g, 0.0))


def ulp32(x):
    """float32 spacing at |x| (values at or above 1 - 2^-24 count as just below 1)"""
    a = np.minimum(np.abs(np.asarray(x, np.float64)), 3e38)
    return np.spacing(a.astype(np.float32)).astype(np.float64)


def element_bounds(cf, t, da, eps):
    """The derived float32 bounds of logp [B], dmu and dls [B, A] around closed_form's values (module docstring, LEVEL A)."""
    t, da, eps = (np.asarray(x, np.float64) for x in (t, da, eps))
    omt, sd, z, aob = cf["omt"], cf["sd"], cf["z"], cf["aob"]
    d_omt = 2.0 ** -23
    dz = ulp32(cf["u"]) / (sd + EPS)
    logp = (d_omt / (omt + EPS) + np.abs(z) * dz + 0.5 * dz * dz).sum(1) + 1e-5 * (1.0 + np.abs(cf["logp"]))
    dmu = np.abs(da) * d_omt + aob * 2.0 * np.abs(t) * EPS / (omt + EPS) ** 2 * d_omt + 8 * E * (np.abs(cf["dmu_q"]) + np.abs(cf["dmu_lp"]))
    dls = np.abs(eps * sd) * dmu + 32 * E * (np.abs(cf["dls_u"]) + np.abs(cf["dls_g"]))
    return dict(logp=logp, dmu=dmu, dls=dls)


def _excess(got, ref, bound, what):
    d = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(got).all(), what + " is not finite"
    over = d - bound
    i = np.unravel_index(np.argmax(over), over.shape)
    assert over[i] <= 0, "%s: |d| %.3e at %s exceeds the bound %.3e (value %.9g, reference %.9g)" % (what, d[i], i, bound[i], got[i], ref[i])


def _rel(got, ref, rel, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    assert (d <= rel * np.abs(ref)).all(), "%s: %s against %s (relative %.3e)" % (what, got, ref, (d / np.maximum(np.abs(ref), 1e-300)).max())


# --------------------------------------------------------------------------------------------------- level A
def fetch_rows(eng, name, B, A):
    """[B, A] of a buffer whose rows may be padded to a multiple of 4 columns; the padding must be zero"""
    raw = eng.fetch(name)
    assert raw.size % B == 0 and raw.size // B >= A, (name, raw.size)
    x = raw.reshape(B, raw.size // B)
    assert not x[:, A:].any(), name + ": padding columns are not zero"
    return x[:, :A].copy()


def check_elements(eng, case):
    """LEVEL A after exactly one update on the case's first minibatch.  Returns the figures it measured."""
    spec, B, A, regime = case["spec"], case["B"], case["spec"].act_dim, case["regime"]
    eps = case["eps"][0]
    assert np.array_equal(eng.fetch("act", (B, A)), batch_of(case, 0)["act"].numpy())
    mu, ls, pi, da = (eng.fetch(n, (B, A)) for n in ("mu", "log_std", "pi", "da_pi"))
    logp = eng.fetch("logp", (B,))
    dmu, dls = fetch_rows(eng, "dmu", B, A), fetch_rows(eng, "dls", B, A)
    log_alpha = np.float64(case["params"]["model/log_ent_coef:0"])        # (the update's own, not the one Adam has moved since)
    assert np.float32(log_alpha) == LOG_ENT_COEF
    alpha = float(np.exp(log_alpha))

    # pi against float64 tanh of the engine's own mu and log-std
    u64 = mu.astype(np.float64) + eps.astype(np.float64) * np.exp(np.clip(ls.astype(np.float64), osac.LOG_STD_MIN, osac.LOG_STD_MAX))
    t64, omt64 = np.tanh(u64), sech2(u64)
    sd64 = np.exp(np.clip(ls.astype(np.float64), osac.LOG_STD_MIN, osac.LOG_STD_MAX))
    du = omt64 * (ulp32(u64) + np.abs(eps * sd64) * 2.0 ** -23)
    ulp_t = ulp32(np.minimum(np.abs(t64), 1.0 - E))
    worst = float(((np.abs(pi - t64) - du) / ulp_t).max())
    WORST["pi_ulp"] = max(WORST["pi_ulp"], worst)
    _excess(pi, t64, K_ULP * ulp_t + du, "pi")

    # logp, dmu, dls against the closed form at the engine's own pi
    cf = closed_form(mu, ls, eps, pi, da, alpha, B)
    bd = element_bounds(cf, pi, da, eps)
    _excess(logp, cf["logp"], bd["logp"], "logp")
    _excess(dmu, cf["dmu"], bd["dmu"], "dmu")
    _excess(dls, cf["dls"], bd["dls"], "dls")
    outside = ~cf["inside"]
    assert (dls.view(np.uint32)[outside] == 0).all(), "dls of an element outside the clip is not +0.0"
    sat = np.abs(u64) >= 15.0
    assert (pi[sat] == np.sign(u64[sat]).astype(np.float32)).all(), "a saturated element's pi is not +-1"
    assert (dmu[sat] == 0.0).all(), "a saturated element has a mu-gradient"
    if regime == "saturated":
        assert sat.any() and np.isfinite(logp).all()
    if regime in ("clip", "combined"):
        assert outside[:, 2].all() and outside[:, 3].all() and not outside[:, :2].any()
        assert outside[:, 4].any() and not outside[:, 4].all() or B < 2

    # hand-over to the weight gradients
    G = eng.get_gradients()
    for n, x in (("model/pi/dense/bias:0", dmu.astype(np.float64)), ("model/pi/dense_1/bias:0", dls.astype(np.float64))):
        d = np.abs(G[n] - x.sum(0))
        assert (d <= 1e-5 * np.abs(x).sum(0)).all(), "gradient of %s: %s against the column sums %s" % (n, G[n], x.sum(0))
    if regime in ("clip", "combined"):
        for j in (2, 3):
            assert not G["model/pi/dense_1/kernel:0"][:, j].any() and G["model/pi/dense_1/bias:0"][j] == 0.0, "column %d is outside the clip in every row" % j

    # loss scalars and the gradient of log_ent_coef from the engine's own rows
    f = {n: eng.fetch(n, (B,)).astype(np.float64) for n in ("v", "qf1_pi", "qf2_pi", "qf1", "qf2", "v_tgt", "rew", "done")}
    lp = logp.astype(np.float64)
    qb = f["rew"] + (1.0 - f["done"]) * spec.gamma * f["v_tgt"]
    vb = np.minimum(f["qf1_pi"], f["qf2_pi"]) - alpha * lp
    want = {"policy_loss": np.mean(alpha * lp - f["qf1_pi"]), "value_loss": 0.5 * np.mean((f["v"] - vb) ** 2),
            "qf1_loss": 0.5 * np.mean((qb - f["qf1"]) ** 2), "qf2_loss": 0.5 * np.mean((qb - f["qf2"]) ** 2),
            "ent_coef_loss": -log_alpha * np.mean(lp + spec.target_entropy), "ent_coef": alpha}
    assert want["ent_coef_loss"] != 0.0 and abs(alpha - 0.2) < 1e-7
    m = eng.metrics()
    for k, ref in want.items():
        _rel(m[k], ref, 1e-5, k)
    _rel(G["model/log_ent_coef:0"], -np.mean(lp + spec.target_entropy), 1e-5, "gradient of log_ent_coef")
    return {"pi_ulp": worst}


# --------------------------------------------------------------------------------------------------- level B
class _PolicyOnly:
    """the oracle's policy group alone, for parity_util.compare_params"""

    def __init__(self, orc):
        names = set(orc.groups[0])
        self.P = OrderedDict((n, v) for n, v in orc.P.items() if n in names)
        self.opt = [orc.opt[0]]


def check_end_to_end(eng, case, train_second):
    """LEVEL B.  The engine has done one update on the first minibatch; `train_second()` does the second."""
    spec, B, A, regime = case["spec"], case["B"], case["spec"].act_dim, case["regime"]
    assert regime in WELL_CONDITIONED
    d0, orc = case["ref64"][0], case["orc64"]
    assert orc.dtype == torch.float64 and d0["mu"].dtype == np.float64
    pu.close(eng.fetch("mu", (B, A)), d0["mu"], what="mu")
    for name in ("qf1", "qf2", "v", "v_tgt") + (() if regime == "small_sd" else ("qf1_pi", "qf2_pi")):
        pu.close(eng.fetch(name, (B,)), d0[name], what=name)
    g_pi, g_vf, _ = orc.groups
    G = eng.get_gradients()
    for n in g_pi + ([] if regime == "small_sd" else g_vf):
        pu.close_rel_max(G[n], d0["grads"][n], what="grad " + n)
    train_second()
    pu.compare_params(eng, _PolicyOnly(orc) if regime == "small_sd" else orc, spec.lr, 2)


# --------------------------------------------------------------------------------------------------- routes
def head_route(dump):
    """Which of the three head routes the plan of a handle launches, from the tags of its GRL_PLAN_DUMP `seq ops_grads` line."""
    lines = [l for l in dump.splitlines() if l.startswith("grl plan: seq ops_grads ")]
    assert lines, dump
    tags = lines[-1].split()[4:]
    if "heads" in tags:
        assert not {"heads_fwd", "heads_bwd", "sample", "sample_bwd", "sac_loss"} & set(tags), tags
        return "one_launch"
    if "sample" in tags:
        assert {"sample_bwd", "sac_loss", "heads_fwd", "heads_bwd"} <= set(tags), tags
        return "per_layer"
    assert tags.count("heads_fwd") == 1 and tags.count("heads_bwd") == 1, tags
    return "chains"


# --------------------------------------------------------------------------------------------------- acting
def check_act(eng, case, rows_list=(1, 17)):
    """Deterministic and stochastic actions against the float64 oracle's tanh(mu + exp(clip(ls)) eps).  The clipped columns get
    UNSCALED noise here: a missing upper clip shows as e^2.5 against e^2; exp(-25) against exp(-20) is invisible either way, so
    the lower clip is judged on the training side only."""
    spec = case["spec"]
    orc = osac.SacOracle(spec, case["params"], dtype=torch.float64)
    st, cap = case["stats"], case["cfg"].act_batch
    rng = np.random.default_rng(5)
    for rows in rows_list:
        assert rows <= cap
        raw = np.concatenate([case["tr"]["obs"]] * (rows // len(case["tr"]["obs"]) + 1))[:rows]
        obs = osac.normalize_obs(raw, st["mean"], st["var"]).astype(np.float32)
        eps = rng.standard_normal((rows, spec.act_dim)).astype(np.float32)
        pu.close(eng.act(obs, True), orc.act(obs, True), what="deterministic action, %d rows" % rows)
        pu.close(eng.act(obs, False, eps), orc.act(obs, False, eps), what="stochastic action, %d rows" % rows)


def state_of(eng):
    P = eng.get_parameters()
    return [P[n] for n in P] + [eng.fetch("adam_m").copy(), eng.fetch("adam_v").copy()]


# --------------------------------------------------------------------------------------------------- what both engine files run
# (shape, switch) -> the head route its plan must launch.  Layers wider than 64 (other than [128, 128]) are outside the one-launch
# matrix-core kernel, so at (96, 72) the default plan already IS the VALU chains and GRL_NO_HEADS_MFMA changes nothing; the
# one-launch route runs the same batch and action widths at (48, 40).
SWITCHES = {None: None, "no_heads_mfma": ("GRL_NO_HEADS_MFMA", "1"), "no_fused_heads": ("GRL_NO_FUSED_HEADS", "1")}
ROUTE = {("mlp_96_72", None): "chains", ("mlp_96_72", "no_heads_mfma"): "chains", ("mlp_96_72", "no_fused_heads"): "per_layer",
         ("mlp_48_40", None): "one_launch", ("mlp_260", None): "per_layer", ("augmented", None): "one_launch", ("mlp_b1", None): "one_launch"}
ALL4 = ("clip", "saturated", "near_saturated", "small_sd")
ELEMENT_RUNS = ([("mlp_96_72", sw, r) for sw in (None, "no_heads_mfma", "no_fused_heads") for r in ALL4] + [("mlp_48_40", None, r) for r in ALL4] +
                [(s, None, r) for s in ("mlp_260", "augmented") for r in ("clip", "saturated")] + [("mlp_b1", None, "saturated")])
END_TO_END_RUNS = [run for run in ELEMENT_RUNS if run[2] in WELL_CONDITIONED]
ACT_RUNS = [(shape, tune, r) for shape, tune in (("act_64_64", None), ("act_64_64", "act_mfma=0"), ("act_260", None)) for r in ("clip", "saturated")]
run_id = lambda run: "-".join(str(x) for x in run if x)


def start(case, switch, monkeypatch, capfd, **engine_kw):
    """A handle for the case under the switch, after its first update; its head route is the one ROUTE names."""
    for var, _ in filter(None, SWITCHES.values()):
        monkeypatch.delenv(var, raising=False)
    if SWITCHES[switch]:
        monkeypatch.setenv(*SWITCHES[switch])
    monkeypatch.setenv("GRL_PLAN_DUMP", "1")
    capfd.readouterr()
    eng = pu.engine_setup(case, **engine_kw)
    dump = capfd.readouterr().err
    monkeypatch.delenv("GRL_PLAN_DUMP")
    assert head_route(dump) == ROUTE[(case["shape"], switch)], dump
    eng.train(1, case["idx"][:1], case["eps"][:1])
    return eng


def run_elements(run, monkeypatch, capfd, **engine_kw):
    shape, switch, regime = run
    case = case_with_reference(shape, regime)
    eng = start(case, switch, monkeypatch, capfd, **engine_kw)
    try:
        check_elements(eng, case)
    finally:          # (the figure behind K_ULP: printed before anything asserts on it)
        print("sac edge %s: tanhf worst so far %.3f ulp beyond the rounding of u" % (run_id(run), WORST["pi_ulp"]))
    eng.close()


def run_end_to_end(run, monkeypatch, capfd, **engine_kw):
    shape, switch, regime = run
    case = case_with_reference(shape, regime)
    eng = start(case, switch, monkeypatch, capfd, **engine_kw)
    check_end_to_end(eng, case, lambda: eng.train(1, case["idx"][1:2], case["eps"][1:2]))
    eng.close()


def run_act(run, monkeypatch, **engine_kw):
    shape, tune, regime = run
    monkeypatch.delenv("GRL_TUNE", raising=False)
    if tune:
        monkeypatch.setenv("GRL_TUNE", tune)
    case = make_case(shape, regime, n_steps=1, act_batch=17)
    eng = pu.engine_setup(case, **engine_kw)
    check_act(eng, case, (1, 17))
    eng.close()


def run_behaviour_cloning(**engine_kw):
    """One behaviour-cloning update at mlp (96, 72), A = 7, 17 rows, with the mu biases of `saturated`: det = +-1 exactly and the
    (1 - det^2) factor makes dmu exactly 0 on those columns; loss, det and gradients to bc_util's tolerances."""
    import bc_util as bu
    A = 7
    case = bu.make_case("mlp_b17_tail3", obs_dim=29, layers=(96, 72), A=A, B=32, bc_batch=17, absent=0, data_seed=BC_DATA_SEED)
    c = columns("saturated", A)
    case["params"]["model/pi/dense/bias:0"] = np.asarray(c["mu_bias"], np.float32)
    sat = [j for j in range(A) if c["mu_bias"][j] != 0]
    eng = pu.engine_setup(case, **engine_kw)
    bu.check_update(eng, case)
    eng.set_parameters(case["params"])
    table = bu.begin(eng, case)
    eng.bc_train(table, case["bc_idx"][:1])
    det = eng.fetch("bc_det", (17, A))
    dmu = eng.fetch("bc_dmu", (17, (A + 3) // 4 * 4))[:, :A]
    G = eng.get_gradients()
    eng.bc_end()
    assert (det[:, sat] == np.sign(np.asarray(c["mu_bias"], np.float32)[sat])).all(), "det of a saturated column is not +-1"
    assert (dmu[:, sat] == 0.0).all(), "a saturated column has a mu-gradient"
    free = [j for j in range(A) if j not in sat]
    assert dmu[:, free].all()
    assert not G["model/pi/dense/kernel:0"][:, sat].any() and not G["model/pi/dense/bias:0"][sat].any()
    eng.close()


BC_DATA_SEED = 2          # the first data seed at which bc_util.assert_no_sign_ambiguity holds for this case


def run_call_of_three_equals_three_calls(**engine_kw):
    case = make_case("mlp_96_72", "combined", n_steps=3)
    out = []
    for split in ([3], [1, 1, 1]):
        eng = pu.engine_setup(case, **engine_kw)
        k = 0
        for n in split:
            eng.train(n, case["idx"][k:k + n], case["eps"][k:k + n])
            k += n
        out.append(state_of(eng))
        eng.close()
    assert len(out[0]) == len(out[1]) and all(np.array_equal(a, b) for a, b in zip(*out))
    assert all(np.isfinite(a).all() for a in out[0]), "a parameter or an Adam moment is not finite after three updates"
    P0 = list(case["params"].values())
    assert any(not np.array_equal(a, b) for a, b in zip(out[0], P0))


def run_graph_replay_equals_eager(monkeypatch, **engine_kw):
    case = make_case("mlp_96_72", "combined", n_steps=3)
    out = []
    for flag in ("0", "1"):
        monkeypatch.setenv("GRL_NO_GRAPH", flag)
        eng = pu.engine_setup(case, **engine_kw)
        eng.train(3, case["idx"], case["eps"])
        out.append(state_of(eng))
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert all(np.isfinite(a).all() for a in out[0])
